"""CPU: the host half of the GPT.forward evaluation pass (genvc_amd.layers.gpt.forward_eval_prepare / perceiver_key_mask) against what the
reference prepared (captured by hooks, tests/golden/forward_eval_*.npz), and the CPU restatement tests/forward_oracle.py against the
reference's outputs -- before any GPU test trusts either."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from genvc_amd import config as gcfg
from genvc_amd import synth

import forward_oracle as FO

_cache = {}


def case(gold, tag):
    if tag not in _cache:
        _cache.clear()
        from genvc_amd.layers.gpt import forward_eval_prepare
        g = FO.load(gold, tag)
        dims = gcfg.gpt_dims(FO.CASES[tag])
        w = synth.make_weights(int(g["seed"]), synth.gpt_weight_spec(dims))
        x = FO.inputs(g, dims)
        prep = forward_eval_prepare(x["text"], x["text_lengths"], x["codes"], x["wav_lengths"])
        _cache[tag] = (g, dims, w, x, prep)
    return _cache[tag]


@pytest.mark.parametrize("tag", list(FO.CASES))
def test_prepared_ids_targets_and_masks_equal_the_reference(gold, tag):
    g, dims, w, x, prep = case(gold, tag)
    assert np.array_equal(prep["text_ids"].numpy(), g["text_ids"])
    assert np.array_equal(prep["code_ids"].numpy(), g["code_ids"])
    assert np.array_equal(prep["text_targets"].numpy(), g["text_targets"])
    assert np.array_equal(prep["mel_targets"].numpy(), g["mel_targets"])
    Lt = g["text_ids"].shape[1]
    km = prep["key_mask"].numpy()
    assert km.dtype == np.bool_ and int(g["n_cond"]) == 32 and km[:, :32].all()
    assert np.array_equal(km[:, 32:32 + Lt], g["attn_mask_text"]) and np.array_equal(km[:, 32 + Lt:], g["attn_mask_mel"])
    # the shapes the issue asks for: more than 16 consecutive padded keys, a mask edge inside a 16-key tile, 99 rows per item
    assert km.shape[1] == 99 and (~km[1]).sum() > 16 + 16 and int(g["count"]) == 47
    assert (prep["mel_targets"] >= 0).sum() == 47 and (prep["text_targets"] >= 0).sum() == 40 + 5 + 23 + 3


def test_prepare_rejects_what_the_reference_asserts():
    from genvc_amd.layers.gpt import forward_eval_prepare
    text, codes = torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ValueError):
        forward_eval_prepare(text, torch.tensor([5, 2]), codes, torch.tensor([1024, 2048]))          # gpt.py:420-422
    with pytest.raises(ValueError):
        forward_eval_prepare(text + 300, torch.tensor([4, 2]), codes, torch.tensor([1024, 2048]))
    with pytest.raises(ValueError):
        forward_eval_prepare(text, torch.tensor([4, 2]), codes + 2000, torch.tensor([1024, 2048]))
    p = forward_eval_prepare(text, torch.tensor([4, 2]), codes, torch.tensor([1, 3000]))             # codes zero-padded to max + 3, :413-414
    assert p["code_ids"].shape == (2, 8) and p["code_ids"][0].tolist() == [1024, 0, 1025, 1025, 1025, 1025, 1025, 1025]
    assert p["key_mask"][0, 32 + 6:].tolist() == [True] * 5 + [False] * 3            # l = 1 + 3: positions > 4


def test_perceiver_mask_keeps_the_reference_misalignment(gold):
    from genvc_amd.layers.gpt import perceiver_key_mask
    g = FO.load(gold, "tiny")
    lens = torch.from_numpy(g["cond_lens"]) // 256
    m = perceiver_key_mask(lens, FO.COND_FRAMES)
    assert np.array_equal(m.numpy(), g["perceiver_mask"]) and m.shape == (3, 332)
    assert lens.tolist() == [300, 40, 20]
    # entry j meets key j of [32 latents | 300 frames]: masked keys are [len, 300) -- latents 20..31 for the third item --, and the
    # last 32 frames (keys 300..331) are always attended
    assert m[:, 300:].all() and m[0].all() and not m[1, 40:300].any() and not m[2, 20:300].any() and m[2, :20].all()


@pytest.mark.parametrize("tag", list(FO.CASES))
def test_restatement_matches_the_reference(gold, tag):
    g, dims, w, x, prep = case(gold, tag)
    ids = torch.from_numpy(g["vocab_ids"])
    # the screen the fixture was kept under
    assert float(g["margin"]) >= FO.MIN_MARGIN
    for ls, sfx in ((0.0, "ls0"), (0.1, "ls1")):
        lt, lm, hits, n, ml = FO.forward(w, dims, prep, x["cond"], ls)
        assert abs(lt - float(g["loss_text_" + sfx])) < 2e-4 and abs(lm - float(g["loss_mel_" + sfx])) < 2e-4
    assert (hits, n) == (int(g["hits"]), int(g["count"])) and 0 < hits < n
    np.testing.assert_allclose(ml[:, ids].numpy(), g["mel_logits_sub"], atol=1e-4)
    if "mel_logits" in g:
        np.testing.assert_allclose(ml.numpy(), g["mel_logits"], atol=1e-4)
    # masked get_style_emb, then the end-to-end call
    from genvc_amd.layers.gpt import perceiver_key_mask
    style = FO.perceiver(w, x["mels"].permute(0, 2, 1), perceiver_key_mask(x["cond_lens"] // 256, FO.COND_FRAMES))
    st = style.transpose(1, 2)
    np.testing.assert_allclose((st if tag == "tiny" else st[:, ::8]).numpy(), g["style"], atol=2e-5)
    lt, lm, hits, n, ml = FO.forward(w, dims, prep, style)
    assert abs(lt - float(g["e2e_loss_text"])) < 2e-4 and abs(lm - float(g["e2e_loss_mel"])) < 2e-4
    assert (hits, n) == (int(g["e2e_hits"]), int(g["e2e_count"]))
    np.testing.assert_allclose(ml[:, ids].numpy(), g["e2e_mel_logits_sub"], atol=1e-4)
    # ragged return_latent=True: the same padding, no mask, the last five rows dropped
    Lt = prep["text_ids"].shape[1]
    rel = FO.latents(w, dims, x["cond"], prep["text_ids"], prep["code_ids"])[:, Lt:][:, :-5]
    np.testing.assert_allclose((rel if tag == "tiny" else rel[:, :, ::8]).numpy(), g["relatents"], atol=1e-4)


def test_loss_and_rank_reduction_against_torch(gold):
    g, dims, w, x, prep = case(gold, "tiny")
    ml = torch.from_numpy(g["mel_logits"])
    t = prep["mel_targets"]
    for ls in (0.0, 0.1):
        ref = float(F.cross_entropy(ml.double(), t, ignore_index=-1, label_smoothing=ls))
        got, hits, n = FO.loss_and_hits(ml.permute(0, 2, 1).reshape(-1, ml.shape[1]), t.reshape(-1), ls)
        assert abs(got - ref) < 1e-9
    rows, tt = ml.permute(0, 2, 1).reshape(-1, ml.shape[1])[t.reshape(-1) >= 0], t.reshape(-1)[t.reshape(-1) >= 0]
    in_top = (rows.topk(10, dim=1)[1] == tt[:, None]).any(1)
    assert int(in_top.sum()) == hits == int(g["hits"]) and n == 47
