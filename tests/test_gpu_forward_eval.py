"""GPU: the evaluation pass of GPT.forward (reference layers/gpt.py:375-537) -- ragged batches, both losses, top-10 accuracy, mel logits --
against the reference's outputs (tests/golden/forward_eval_*.npz, scripts/make_forward_golden.py) and the CPU restatement
tests/forward_oracle.py (pinned against the same fixtures by test_forward_eval_host.py)."""
import numpy as np
import pytest
import torch

from genvc_amd import config as gcfg
from genvc_amd import synth

import forward_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAGS = list(FO.CASES)
_cache = {}

# End-to-end logits tolerance per case: what the CPU restatement's mel logits move by when its conditioning latents are perturbed by
# 5e-5 (the bar of the masked get_style_emb below) with random signs -- the largest of four draws, measured on the CPU for these shapes:
# tiny 3.4e-5, hd256 6.7e-5, hd64 7.4e-5.  The losses get twice that.
E2E_LOGITS_TOL = {"tiny": 3.4e-5, "hd256": 6.8e-5, "hd64": 7.4e-5}


def case(gold, tag, **init):
    key = (tag, tuple(sorted(init.items())))
    if key not in _cache:
        from genvc_amd.layers.gpt import GPT, forward_eval_prepare
        a = FO.CASES[tag]
        g = FO.load(gold, tag)
        dims = gcfg.gpt_dims(a)
        w = synth.make_weights(int(g["seed"]), synth.gpt_weight_spec(dims))
        m = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"], max_text_tokens=a["gpt_max_text_tokens"],
                max_mel_tokens=a["gpt_max_audio_tokens"], max_prompt_tokens=a["gpt_max_prompt_tokens"])
        missing, unexpected = m.load_state_dict(w, strict=False)
        assert not missing and not unexpected
        m = m.to(DEV).eval()
        m.init_gpt_for_inference(**dict(dict(max_slots=4, max_rows=1024), **init))
        x = FO.inputs(g, dims)
        prep = forward_eval_prepare(x["text"], x["text_lengths"], x["codes"], x["wav_lengths"])
        _cache[key] = (g, dims, w, m, x, prep)
    return _cache[key]


def call(m, x, **kw):
    return m(x["text"].to(DEV), x["text_lengths"], x["codes"].to(DEV), x["wav_lengths"], **kw)


def sub(g, tag, t):
    return t if tag == "tiny" else t[:, torch.from_numpy(g["vocab_ids"])]


@pytest.mark.parametrize("tag", TAGS)
def test_gpt_only_call_matches_the_reference(gold, tag):
    g, dims, w, m, x, prep = case(gold, tag)
    assert float(g["margin"]) >= FO.MIN_MARGIN            # every target logit is >= 2e-3 away from the 10th / 11th boundary
    for ls, sfx in ((0.0, "ls0"), (0.1, "ls1")):
        m.label_smoothing = ls
        lt, lm, acc, ml = call(m, x, cond_latents=x["cond"].to(DEV))
        assert lt.shape == () and lm.shape == () and lt.dtype == torch.float32 and ml.shape == (3, 1026, 25) and not ml.is_contiguous()
        err = float((sub(g, tag, ml.cpu()) - torch.from_numpy(g["mel_logits" if tag == "tiny" else "mel_logits_sub"])).abs().max())
        print(f"{tag} ls {ls}: logits err {err:.2e}, loss_text {float(lt) - float(g['loss_text_' + sfx]):+.2e}, "
              f"loss_mel {float(lm) - float(g['loss_mel_' + sfx]):+.2e}, acc {float(acc):.4f}")
        assert err <= 1e-4                                 # every column, the padded ones included
        assert abs(float(lt) - float(g["loss_text_" + sfx])) <= 2e-4 and abs(float(lm) - float(g["loss_mel_" + sfx])) <= 2e-4
        assert round(float(acc) * int(g["count"])) == int(g["hits"]) and abs(float(acc) - int(g["hits"]) / int(g["count"])) < 1e-6
    m.label_smoothing = 0.0


@pytest.mark.parametrize("tag", TAGS)
def test_masked_style_emb_matches_the_reference(gold, tag):
    g, dims, w, m, x, prep = case(gold, tag)
    st = m.get_style_emb(x["mels"].to(DEV), seq_lens=x["cond_lens"] // 256).cpu()
    assert st.shape == (3, dims["d_model"], 32)
    np.testing.assert_allclose((st if tag == "tiny" else st[:, ::8]).numpy(), g["style"], atol=5e-5)


@pytest.mark.parametrize("tag", TAGS)
def test_end_to_end_call_matches_the_reference(gold, tag):
    g, dims, w, m, x, prep = case(gold, tag)
    tol = E2E_LOGITS_TOL[tag]
    lt, lm, acc, ml = call(m, x, cond_mels=x["mels"].unsqueeze(1).to(DEV), cond_lens=x["cond_lens"])
    err = float((ml.cpu()[:, torch.from_numpy(g["vocab_ids"])] - torch.from_numpy(g["e2e_mel_logits_sub"])).abs().max())
    print(f"{tag} end to end: logits err {err:.2e} (tol {tol:.1e}), loss_text {float(lt) - float(g['e2e_loss_text']):+.2e}, "
          f"loss_mel {float(lm) - float(g['e2e_loss_mel']):+.2e}")
    assert err <= tol
    assert abs(float(lt) - float(g["e2e_loss_text"])) <= 2 * tol and abs(float(lm) - float(g["e2e_loss_mel"])) <= 2 * tol
    assert round(float(acc) * int(g["e2e_count"])) == int(g["e2e_hits"])


def test_masked_perceiver_keys_have_exactly_zero_weight(gold):
    """the reference's mask meets key j of [32 latents | frames] (a misalignment that is reproduced): item 1 (40 frames of 300) masks
    keys [40, 300) = frames 8 .. 267, and the last 32 frames are attended although they lie beyond its length"""
    g, dims, w, m, x, prep = case(gold, "tiny")
    lens = x["cond_lens"] // 256
    base = m.get_style_emb(x["mels"].to(DEV), seq_lens=lens)
    inside = x["mels"].clone()
    inside[1, :, 8:268] += 1.0
    assert torch.equal(m.get_style_emb(inside.to(DEV), seq_lens=lens), base)
    tail = x["mels"].clone()
    tail[1, :, 268:] += 1.0
    moved = m.get_style_emb(tail.to(DEV), seq_lens=lens)
    assert torch.equal(moved[0], base[0]) and torch.equal(moved[2], base[2])
    assert float((moved[1] - base[1]).abs().max()) > 1e-3


@pytest.mark.parametrize("tag", TAGS)
def test_masked_gpt_keys_have_exactly_zero_weight(gold, tag):
    """ids under masked text keys (item 1: positions 6 .. 41, more than two whole 16-key tiles) change: the code rows behind them, which
    see every text key but the masked ones, stay bit-identical; without the mask they move"""
    g, dims, w, m, x, prep = case(gold, tag)
    slots = torch.arange(3, device=DEV, dtype=torch.int32)
    cond, km = x["cond"].to(DEV), prep["key_mask"].to(DEV)
    Lt = prep["text_ids"].shape[1]
    other = prep["text_ids"].clone()
    other[1, 6:] = 7
    assert not prep["key_mask"][1, 32 + 6:32 + Lt].any()
    run = lambda ids, mask: m.engine.forward_rows(slots, cond, ids.to(DEV).int(), prep["code_ids"].to(DEV).int(), mask)
    a, b = run(prep["text_ids"], km), run(other, km)
    assert torch.equal(a[:, Lt:], b[:, Lt:]) and torch.equal(a[1, :6], b[1, :6]) and not torch.equal(a[1, 6:Lt], b[1, 6:Lt])
    assert not torch.equal(run(prep["text_ids"], None)[1, Lt:], run(other, None)[1, Lt:])


@pytest.mark.parametrize("tag", TAGS)
def test_each_item_alone_equals_its_rows_of_the_ragged_batch(gold, tag):
    g, dims, w, m, x, prep = case(gold, tag)
    _, _, _, ml = call(m, x, cond_latents=x["cond"].to(DEV))
    for b in range(3):
        tl, n = int(x["text_lengths"][b]), int(prep["code_lengths"][b]) - 3
        _, _, _, one = m(x["text"][b:b + 1, :tl].to(DEV), x["text_lengths"][b:b + 1], x["codes"][b:b + 1, :n].to(DEV),
                         x["wav_lengths"][b:b + 1], cond_latents=x["cond"][b:b + 1].to(DEV))
        assert one.shape == (1, 1026, n + 5)
        np.testing.assert_allclose(one[0].cpu().numpy(), ml[b, :, :n + 5].cpu().numpy(), atol=1e-4)


@pytest.mark.parametrize("tag", TAGS)
def test_long_rows_with_scattered_masks_match_the_restatement(gold, tag):
    """172 rows per item: beyond the 128 keys of the short tile kernel, so the chunked one runs -- mask edges inside a tile and on a tile
    boundary, a fully masked 16-key tile, masked keys across the 64-key V chunk boundary"""
    g, dims, w, m, x, prep = case(gold, tag)
    B, Lt, Lm = 2, 100, 40
    seed = int(g["seed"])
    text = synth.integers(seed, "fe_long_text", (B, Lt), 258)
    codes = synth.integers(seed, "fe_long_codes", (B, Lm), 1026)
    km = torch.ones(B, 32 + Lt + Lm, dtype=torch.bool)
    km[0, 48:64] = False            # one whole tile
    km[0, 70:75] = False            # inside a tile
    km[0, 120:136] = False          # across the 128-key / V-chunk boundary
    km[1, 37:112] = False           # four whole tiles and two edges, one of them on a tile boundary
    km[1, 150:] = False             # the tail
    ref = FO.latents(w, dims, x["cond"][:B], text, codes, km)
    got = m.engine.forward_rows(torch.arange(B, device=DEV, dtype=torch.int32), x["cond"][:B].to(DEV), text.to(DEV).int(),
                                codes.to(DEV).int(), km.to(DEV))
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), atol=1e-4)


def test_two_identical_calls_return_identical_bits(gold):
    g, dims, w, m, x, prep = case(gold, "hd256")
    a = call(m, x, cond_latents=x["cond"].to(DEV))
    b = call(m, x, cond_latents=x["cond"].to(DEV))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("tag", TAGS)
def test_ragged_return_latent_matches_the_reference(gold, tag):
    g, dims, w, m, x, prep = case(gold, tag)
    rel = call(m, x, cond_latents=x["cond"].to(DEV), return_latent=True).cpu()
    assert rel.shape == (3, 20, dims["d_model"])
    np.testing.assert_allclose((rel if tag == "tiny" else rel[:, :, ::8]).numpy(), g["relatents"], atol=1e-4)


def test_equal_length_return_latent_is_the_existing_pass(gold):
    g, dims, w, m, x, prep = case(gold, "tiny")
    text, codes, cond = x["text"][:2, :9].to(DEV), x["codes"][:2, :12].to(DEV), x["cond"][:2].to(DEV)
    got = m(text, torch.tensor([9, 9]), codes, torch.tensor([12 * 1024, 12 * 1024 - 5]), cond_latents=cond, return_latent=True)
    prefix = m.engine.prefix_embeddings(cond, text.int())
    assert torch.equal(got, m.engine.latents(torch.arange(2, device=DEV, dtype=torch.int32), prefix, codes.int()))


def test_refusals(gold):
    g, dims, w, m, x, prep = case(gold, "tiny")
    cond = x["cond"].to(DEV)
    with pytest.raises(NotImplementedError):
        call(m, x, cond_latents=cond, return_attentions=True)
    with pytest.raises(ValueError):             # more items than slots
        m(x["text"].repeat(2, 1).to(DEV), x["text_lengths"].repeat(2), x["codes"].repeat(2, 1).to(DEV), x["wav_lengths"].repeat(2),
          cond_latents=cond.repeat(2, 1, 1))
    with pytest.raises(ValueError):             # text rows beyond the position table (404)
        m(torch.zeros(1, 410, dtype=torch.long, device=DEV), torch.tensor([410]), x["codes"][:1].to(DEV), x["wav_lengths"][:1],
          cond_latents=cond[:1])
    with pytest.raises(ValueError):             # code rows beyond the position table (608)
        m(x["text"][:1].to(DEV), x["text_lengths"][:1], torch.zeros(1, 610, dtype=torch.long, device=DEV), torch.tensor([610 * 1024]),
          cond_latents=cond[:1])
    small = case(gold, "tiny", max_rows=256)[3]
    with pytest.raises(ValueError):             # 3 x 99 rows > max_rows
        call(small, x, cond_latents=cond)
    bf16 = case(gold, "tiny", weight_dtype="bf16")[3]
    with pytest.raises(NotImplementedError, match="bf16"):
        call(bf16, x, cond_latents=cond)
