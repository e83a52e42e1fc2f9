"""GPU: contrastive search (include/genvc_hip.h: gvc_gpt_prefill_hidden, gvc_gpt_contrastive_generate) against
tests/golden/contrastive_search.npz (the loop driven on the reference's own forward, scripts/make_contrastive_golden.py) and the CPU
restatement (tests/cs_oracle.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cs_oracle as CO                        # noqa: E402
from oracle import genvc_oracle as O          # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contrastive_search.npz")
EOS = 1025


def make_gpt(model_args, seed, stop_bias=None, max_slots=16, weight_dtype="fp32"):
    from genvc_amd.layers.gpt import GPT
    a = model_args
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    dims = gcfg.gpt_dims(a)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][EOS] = float(stop_bias)
    g.load_state_dict(w, strict=False)
    g.to(DEV)
    g.init_gpt_for_inference(max_slots=max_slots, weight_dtype=weight_dtype)
    return g, w, dims


def fixture_case(gold, tag, **kw):
    full = bool(gold[f"{tag}_full"])
    margs = gcfg.DEFAULT_MODEL_ARGS if full else gcfg.TINY_MODEL_ARGS
    sb = float(gold[f"{tag}_stop_bias"])
    g, w, dims = make_gpt(margs, int(gold[f"{tag}_seed"]), stop_bias=sb if sb != 0.0 else None, **kw)
    g.max_gen_mel_tokens = int(gold[f"{tag}_max_new"])
    B, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(s, "content_codes", (B, Tc), 256).to(DEV)
    gkw = dict(do_sample=False, top_k=int(gold[f"{tag}_K"]), repetition_penalty=float(gold[f"{tag}_rep"]))
    if int(gold[f"{tag}_ngram"]):
        gkw["no_repeat_ngram_size"] = int(gold[f"{tag}_ngram"])
    if int(gold[f"{tag}_min_new"]):
        gkw["min_new_tokens"] = int(gold[f"{tag}_min_new"])
    return g, w, dims, cond, codes, gkw, full


def close(g):
    g.engine.close()
    del g
    torch.cuda.empty_cache()


# ---- 1. GPT.generate reproduces the fixture on both decode classes ----------------------------------------------------------------
@pytest.mark.parametrize("rows_step", ["1", "0"])
def test_generate_matches_fixture(rows_step, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST_ROWS", rows_step)
    gold = dict(np.load(GOLD))
    for tag in ("a", "b", "c", "d", "e"):
        g, _, _, cond, codes, gkw, full = fixture_case(gold, tag)
        for i in range(int(gold[f"{tag}_n"])):
            assert float(gold[f"{tag}_{i}_prob_gap"]) >= 1e-3 and float(gold[f"{tag}_{i}_score_gap"]) >= 1e-4     # the margin screens
            ids = g.generate(cond, codes, penalty_alpha=float(gold[f"{tag}_{i}_alpha"]), group=8, **gkw)
            assert np.array_equal(ids.cpu().numpy(), gold[f"{tag}_{i}_ids"]), (tag, i)
        if full and rows_step == "1":
            assert g.engine.decode_variant() == 5          # B*K = 4 rows on the one-launch rows step
        close(g)


# ---- 2. one step against the restatement on crafted context rows -------------------------------------------------------------------
def crafted_step(w, dims, cond, codes, K, alpha, rep, seed):
    """the restatement of step 0 on context rows the test crafts: the prompt's ln_f rows, with near-duplicates of every candidate's hidden
    row (cosine 1 - eps_k, eps_k a permutation of 1e-2 .. 4e-2 spaced 1e-2) and a second row within 1e-7 of candidate 0's maximum (a
    near-tie of the max over the context), and one prompt row duplicated up to scale.  -> (ctx, candidates, probabilities, k*, scores,
    k* on the uncrafted rows, K-th vs (K+1)-th processed gap)"""
    wc = {k: (v if torch.is_tensor(v) else torch.as_tensor(v)).float() for k, v in w.items()}
    fake, hid, logits, cache = CO.prefill(wc, dims, cond, codes)
    B, n0 = fake.shape
    d = hid.shape[-1]
    s = CO.process_rows(logits, [list(map(int, r)) for r in fake], n0, rep, {}, EOS)
    pk, tk = torch.topk(torch.softmax(s, -1), K, dim=-1)
    gap = float((torch.topk(s, K + 1, dim=-1).values[:, K - 1] - torch.topk(s, K + 1, dim=-1).values[:, K]).min())
    cache = [(k.repeat_interleave(K, 0), v.repeat_interleave(K, 0)) for k, v in cache]
    emb = (wc["mel_embedding.weight"][tk.reshape(-1)] + wc["mel_pos_embedding.emb.weight"][1]).unsqueeze(1)
    h = O.gpt_blocks(wc, dims, emb, cache)[0][:, -1].view(B, K, d)
    gen = torch.Generator().manual_seed(seed)
    ctx = hid.clone()

    def at_cos(v, c):
        v = v / v.norm()
        u = torch.randn(d, generator=gen, dtype=torch.float64)
        u = u - (u @ v) * v
        return c * v + (1.0 - c * c) ** 0.5 * u / u.norm()
    for b in range(B):
        eps = (torch.randperm(K, generator=gen).double() + 1.0) * 1e-2
        for k in range(K):
            ctx[b, 2 + 2 * k] = at_cos(h[b, k].double(), 1.0 - float(eps[k])).float() * (1.5 + k)
        ctx[b, 3] = at_cos(h[b, 0].double(), 1.0 - float(eps[0]) - 1e-7).float() * 0.7
        ctx[b, 1] = ctx[b, 0] * 1.0001
    sel, score = CO.rank(ctx, h, pk, alpha)
    sel0, _ = CO.rank(hid, h, pk, alpha)
    return ctx, tk, pk, sel, score, sel0, gap


def test_one_step_on_crafted_context():
    """recall + similarity + select of one step against the restatement: near-duplicate context rows, a near-tie of the cosine max, an
    eos candidate (the stop token is biased into the top-K) and an item that has already finished (its token is eos whatever wins)"""
    from genvc_amd.engine import ContrastiveSearch
    B, K, alpha, rep = 3, 4, 0.6, 1.0
    g, w, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 61, stop_bias=2.5)
    d = dims["d_model"]
    cond = synth.uniform(6100, "cond_latents", (B, 32, d), 1.0)
    codes = synth.integers(6100, "content_codes", (B, 9), 256)
    fake = g.compute_embeddings(cond.to(DEV), codes.to(DEV))
    slots = torch.arange(B * K, device=DEV, dtype=torch.int32)
    moved = eos_seen = 0
    for seed in range(4):
        ctx, tk, pk, sel, score, sel0, gap = crafted_step(w, dims, cond, codes, K, alpha, rep, seed)
        assert gap >= 1e-3                                                   # the candidates are the same set on both sides
        top2 = torch.topk(score, 2, dim=-1).values
        assert float((top2[:, 0] - top2[:, 1]).min()) >= 1e-4                # (the crafted rows keep the winner clear of fp32 noise)
        moved += int((sel != sel0).sum())
        eos_seen += int((tk == EOS).any(1).sum())
        cs = ContrastiveSearch(fake, K, 8, EOS, 1026, d, alpha, rep)
        g.engine.prefill_hidden(slots[::K].contiguous(), g._prefix, cs.hidden0)
        cs.hidden0.copy_(ctx.to(DEV))
        cs.finished[2] = 1
        g.engine.contrastive_generate(slots, cs, 1)
        torch.cuda.synchronize()
        g.engine.health()
        want = [EOS if b == 2 else int(tk[b, sel[b]]) for b in range(B)]
        n0 = int(fake.shape[1])
        assert cs.tokens[:, 0].cpu().tolist() == want, (seed, sel.tolist(), tk.tolist())
        assert cs.ids[:, n0].cpu().tolist() == want
        assert cs.finished.cpu().tolist() == [int(b == 2 or want[b] == EOS) for b in range(B)]
    assert moved > 0            # the crafted rows change the choice somewhere
    assert eos_seen > 0         # eos was a candidate
    close(g)


# ---- 3. the prefill's hidden rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True])
def test_prefill_hidden_rows_match_oracle(full):
    margs = gcfg.DEFAULT_MODEL_ARGS if full else gcfg.TINY_MODEL_ARGS
    g, w, dims = make_gpt(margs, 3)
    B, Tc = (1, 13) if full else (2, 9)
    cond = synth.uniform(77, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    codes = synth.integers(77, "content_codes", (B, Tc), 256)
    g.compute_embeddings(cond.to(DEV), codes.to(DEV))
    P = g._prefix.shape[1]
    hid = torch.empty(B, P + 1, dims["d_model"], device=DEV)
    g.engine.prefill_hidden(torch.arange(B, device=DEV, dtype=torch.int32), g._prefix, hid)
    torch.cuda.synchronize()
    want = CO.hidden_rows({k: v for k, v in w.items()}, dims, cond, codes)
    torch.testing.assert_close(hid.cpu(), want, rtol=0, atol=1e-4)
    close(g)


# ---- 4. the candidates' slots hold identical K/V, equal to a replay of the chosen ids ---------------------------------------------
@pytest.mark.parametrize("B,K,steps", [(2, 4, 11), (1, 3, 17)])
def test_candidate_slots_hold_the_kv_a_replay_writes(B, K, steps):
    from genvc_amd.engine import ContrastiveSearch
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 43)
    eng = g.engine
    cond = synth.uniform(4300, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(4300, "content_codes", (B, 10), 256).to(DEV)
    fake = g.compute_embeddings(cond, codes)
    prefix = g._prefix
    slots = torch.arange(B * K, device=DEV, dtype=torch.int32)
    cs = ContrastiveSearch(fake, K, 40, EOS, 1026, dims["d_model"], 0.6, 2.0)
    eng.prefill_hidden(slots[::K].contiguous(), prefix, cs.hidden0)
    eng.contrastive_generate(slots, cs, 3)
    eng.contrastive_generate(slots, cs, steps - 3)            # (a second call continues the search)
    torch.cuda.synchronize()
    eng.health()
    toks = cs.tokens[:, :steps].clone()
    spare = torch.tensor([B * K], device=DEV, dtype=torch.int32)
    probe = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    for b in range(B):
        eng.reset(spare)
        eng.prefill(spare, prefix[b:b + 1].contiguous(), want_outputs=False)
        for j in range(steps):
            eng.decode_step(spare, toks[b, j:j + 1].contiguous())
        ref, _ = eng.decode_step(spare, probe)
        for k in range(K):
            got, _ = eng.decode_step(slots[b * K + k:b * K + k + 1].contiguous(), probe)
            torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)
    close(g)


# ---- 5. last_latents against the teacher-forced re-pass ---------------------------------------------------------------------------
def test_last_latents_match_the_repass():
    gold = dict(np.load(GOLD))
    g, _, dims, cond, codes, gkw, _ = fixture_case(gold, "b")
    ids = g.generate(cond, codes, penalty_alpha=float(gold["b_0_alpha"]), **gkw)
    lat = g.last_latents
    assert lat is not None and lat.shape[:2] == ids.shape
    gen = ids[:, (ids[0] != EOS)]
    n = gen.shape[1]
    rep = g(codes, torch.tensor([codes.shape[1]], device=DEV), gen, torch.tensor([n * 1024], device=DEV), cond_latents=cond,
            return_latent=True)
    np.testing.assert_allclose(lat[:, :n].cpu().numpy(), rep.cpu().numpy(), atol=1e-4)
    close(g)


# ---- 6. the ids do not depend on the host's group; the warmed path neither allocates nor captures ---------------------------------
def test_group_independent_and_warm():
    gold = dict(np.load(GOLD))
    g, _, dims, cond, codes, gkw, _ = fixture_case(gold, "c")
    a = float(gold["c_0_alpha"])
    n0 = 32 + int(gold["c_Tc"]) + 3
    K, B = gkw["top_k"], int(gold["c_B"])
    g.engine.warmup_contrastive(B, K, n0 + int(gold["c_max_new"]))
    base = g.engine.lazy_inits()
    outs = [g.generate(cond, codes, penalty_alpha=a, group=grp, **gkw) for grp in (1, 8, 16)]
    assert g.engine.lazy_inits() == base
    for o in outs:
        assert np.array_equal(o.cpu().numpy(), gold["c_0_ids"])
    close(g)


# ---- 7. the refused paths; sampling with penalty_alpha is sampling -----------------------------------------------------------------
def test_refused_paths_and_sampling_unchanged():
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 43, max_slots=8)
    cond = synth.uniform(4300, "cond_latents", (2, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(4300, "content_codes", (2, 10), 256).to(DEV)
    g.max_gen_mel_tokens = 16
    cs = dict(do_sample=False, top_k=4, penalty_alpha=0.6)
    with pytest.raises(NotImplementedError, match="get_generator"):
        next(g.get_generator(g.compute_embeddings(cond, codes), **cs))
    with pytest.raises(NotImplementedError, match="generate_groups"):
        g.generate_groups([(cond, codes)], **cs)
    with pytest.raises(NotImplementedError, match="generate_rolling"):
        g.generate_rolling([(cond, codes)], **cs)
    with pytest.raises(ValueError, match="max_slots"):
        g.generate(cond, codes, do_sample=False, top_k=8, penalty_alpha=0.6)          # 2 x 8 > 8 slots
    with pytest.raises(NotImplementedError, match="16"):
        g.generate(cond, codes, do_sample=False, top_k=17, penalty_alpha=0.6)
    with pytest.raises(ValueError, match="num_return_sequences"):
        g.generate(cond, codes, num_return_sequences=2, **cs)
    samp = dict(do_sample=True, top_k=4, top_p=0.9, temperature=0.8, seed=11)
    a = g.generate(cond, codes, penalty_alpha=0.6, **samp)
    b = g.generate(cond, codes, **samp)
    assert torch.equal(a, b)
    close(g)


# ---- 8. GenVCModel.inference and synthesize_utt ------------------------------------------------------------------------------------
def test_model_inference_and_synthesize_utt():
    from genvc_amd.inference.inference_utils import segments, synthesize_utt
    from genvc_amd.inference.model_init import model_init_synthetic
    cfg = gcfg.default_config(tiny=True)
    m = model_init_synthetic(cfg, seed=1, device=DEV, max_slots=8)[0]
    m.gpt.max_gen_mel_tokens = 30
    src = synth.uniform(402, "src_wav", (1, 16000), 0.3).to(DEV)
    ref = synth.uniform(100, "ref_wav", (1, 24000 * 3), 0.3).to(DEV)
    cond = m.get_gpt_cond_latents(ref, 24000)
    gkw = dict(do_sample=False, top_k=4, penalty_alpha=0.6, repetition_penalty=2.0)
    feat = m.content_extractor.extract_content_features(src)
    codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
    gen = m.gpt.generate(cond, codes, **gkw)[0]
    gen = gen[gen != EOS]
    wav = m.inference(src, cond, generate_kwargs=gkw)
    assert gen.numel() > 0 and wav.shape[-1] == gen.numel() * 4 * 256
    wav2 = m.inference(src, cond, generate_kwargs=gkw, repass_latents=True)
    np.testing.assert_allclose(wav.cpu().numpy(), wav2.cpu().numpy(), atol=1e-4)
    out = synthesize_utt(m, src, ref, seg_len=0.5, return_details=True, generate_kwargs=gkw)
    cond_u = m.get_gpt_cond_latents(ref.to(m.device), m.config.audio.sample_rate)
    want = []
    for seg in segments(src, int(0.5 * m.content_sample_rate), int(0.32 * m.content_sample_rate)):
        f = m.content_extractor.extract_content_features(seg)
        c = m.content_dvae.get_codebook_indices(f.transpose(1, 2))
        t = m.gpt.generate(cond_u, c, **gkw)[0]
        t = t[t != EOS]
        if t.numel():
            want.append(t)
    assert len(out["codes"]) == len(want) >= 1
    for a, b in zip(out["codes"], want):
        assert torch.equal(a, b)
    # the session scheduler decodes one row per stream: it refuses the kwargs, naming itself, with top_k absent too
    from genvc_amd.streaming import StreamSessions
    for kw in (dict(do_sample=False, top_k=4, penalty_alpha=0.6), dict(do_sample=False, penalty_alpha=0.6)):
        with pytest.raises(NotImplementedError, match="StreamSessions"):
            StreamSessions(m, generate_kwargs=kw)


# ---- 9. the reduced-precision storage modes run deterministically ----------------------------------------------------------------
@pytest.mark.parametrize("wd", ["bf16", "bf16_kv", "bf16_act"])
def test_storage_modes_deterministic(wd):
    gold = dict(np.load(GOLD))
    g, _, dims, cond, codes, gkw, _ = fixture_case(gold, "c", weight_dtype=wd)
    a = g.generate(cond, codes, penalty_alpha=0.5, **gkw)
    b = g.generate(cond, codes, penalty_alpha=0.5, **gkw)
    assert torch.equal(a, b) and a.shape[0] == 3 and a.shape[1] >= 1
    assert int(a.min()) >= 0 and int(a.max()) <= EOS
    close(g)
