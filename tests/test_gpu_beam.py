"""GPU: deterministic beam search (include/genvc_hip.h: gvc_beam_select, gvc_gpt_beam_generate) against the CPU restatement
(tests/beam_oracle.py) and against tests/golden/beam_search.npz (the reference's GPT.generate(num_beams=K, do_sample=False) executed,
scripts/make_beam_golden.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "beam_search.npz")
EOS, V = 1025, 1026


def make_gpt(model_args, seed, stop_bias=None, max_slots=16):
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
    g.init_gpt_for_inference(max_slots=max_slots)
    return g, w, dims


def _hyp_set(beam, b):
    n = int(beam.hyp_count[b])
    hs, hl, ht = beam.hyp_score[b].cpu(), beam.hyp_len[b].cpu(), beam.hyp_tok[b].cpu()
    return sorted((float(hs[i]), ht[i, :int(hl[i])].tolist()) for i in range(n))


# ---- 1. one select step against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", [(1, 2), (3, 4), (4, 8), (1, 8), (3, 2)])
@pytest.mark.parametrize("mode", ["4.33", "generated"])
def test_beam_select_matches_restatement(B, K, mode):
    from genvc_amd.engine import BeamSearch, beam_select
    n0, max_new, rep = 7, 12, 2.0
    gen_ = torch.Generator().manual_seed(1000 * B + K)
    fake = torch.randint(0, 1024, (B, n0), generator=gen_)
    fake[:, -1] = 1024
    ranks_seen = set()
    for lp in (0.5, 1.0, 2.0):
        beam = BeamSearch(fake.to(DEV), K, max_new, EOS, V, lp, rep, mode)
        slots = torch.arange(B * K, device=DEV, dtype=torch.int32)
        scores = beam.scores.cpu().clone()
        gen = [[] for _ in range(B * K)]
        hyps = [BO.Hyps(K) for _ in range(B)]
        done = [False] * B
        ids = fake.repeat_interleave(K, 0)
        for t in range(max_new - 1):
            logits = torch.randn(B * K, V, generator=gen_) * 3.0
            logits[:, EOS] += float([9.0, 3.0, 5.0, 1.0, 7.0, 4.0][t % 6])       # eos candidates above and below rank K
            s = BO.log_probs(logits, ids, rep)
            acc = (s + scores[:, None]).view(B, -1)
            for b in range(B):
                if not done[b]:
                    top = torch.topk(acc[b], 2 * K)[1]
                    ranks_seen.update(int(r >= K) for r, i in enumerate(top.tolist()) if i % V == EOS)
            was_done = list(done)
            tok, par, scores, gen, gap = BO.select_step(s, scores, gen, hyps, done, t, n0, K, V, EOS, lp, mode)
            assert gap > 1e-5, f"near-tie in the random case (gap {gap:.2e}): pick another seed"
            beam_select(beam, logits.to(DEV).contiguous(), slots, t)
            beam.steps = t + 1
            torch.cuda.synchronize()
            assert np.array_equal(beam.tokens.cpu().numpy(), tok.numpy()), (t, lp)
            assert np.array_equal(beam.parents.cpu().numpy(), par.numpy()), (t, lp)
            torch.testing.assert_close(beam.scores.cpu(), scores.float(), rtol=1e-5, atol=1e-4)
            assert beam.done.cpu().tolist() == [int(x) for x in done], (t, lp)
            for b in range(B):
                if was_done[b]:
                    continue
                dev_h = _hyp_set(beam, b)
                ref_h = sorted((sc, tk) for sc, tk in hyps[b].items)
                assert [h[1] for h in dev_h] == [h[1] for h in ref_h], (t, lp, b)
                np.testing.assert_allclose([h[0] for h in dev_h], [h[0] for h in ref_h], rtol=1e-5, atol=1e-6)
                assert abs(float(beam.hyp_worst[b]) - (hyps[b].worst if hyps[b].items else 1e9)) <= 1e-5 * max(1.0, abs(hyps[b].worst))
            # the slot permutation: slots stay a permutation; a parent's slot goes to its first child
            sl = slots.cpu().numpy()
            assert sorted(sl.tolist()) == list(range(B * K))
            src = (torch.arange(B).repeat_interleave(K) * K + par).long()
            ids = torch.cat([ids[src], tok[:, None]], 1)
            assert np.array_equal(beam.ids[(t + 1) & 1, :, :n0 + t + 1].cpu().numpy(), ids.numpy())
            if all(done):
                break
    assert ranks_seen == {0, 1}, f"eos candidates seen only at {'rank < K' if 0 in ranks_seen else 'rank >= K'}"


# ---- 2. GPT.generate(num_beams=K) against the executed reference ------------------------------------------------------------------
@pytest.mark.parametrize("rows_step", ["1", "0"])
def test_generate_matches_executed_reference(rows_step, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST_ROWS", rows_step)
    gold = dict(np.load(GOLD))
    for tag in ("a", "b", "c"):
        full = bool(gold[f"{tag}_full"])
        margs = gcfg.DEFAULT_MODEL_ARGS if full else gcfg.TINY_MODEL_ARGS
        sb = float(gold[f"{tag}_stop_bias"])
        g, _, dims = make_gpt(margs, int(gold[f"{tag}_seed"]), stop_bias=sb if sb != 0.0 else None)
        g.max_gen_mel_tokens = int(gold[f"{tag}_max_new"])
        B, K, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_K"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
        cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
        codes = synth.integers(s, "content_codes", (B, Tc), 256).to(DEV)
        for i in range(int(gold[f"{tag}_n"])):
            assert float(gold[f"{tag}_{i}_min_gap"]) >= 1e-3                 # the fixture's margin screen
            ids = g.generate(cond, codes, num_beams=K, do_sample=False, length_penalty=float(gold[f"{tag}_{i}_lp"]),
                             repetition_penalty=float(gold[f"{tag}_rep"]), beam_length_mode="generated", group=8)
            assert np.array_equal(ids.cpu().numpy(), gold[f"{tag}_{i}_ids"]), (tag, i)
            np.testing.assert_allclose(g.last_beam_scores.numpy(), gold[f"{tag}_{i}_best_scores"], rtol=1e-4, atol=1e-5)
        if full and rows_step == "1":
            assert g.engine.decode_variant() == 5          # B*K = 4 rows on the one-launch rows step
        g.engine.close()
        del g
        torch.cuda.empty_cache()


# ---- 3. slot permutation and KV span copies ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,steps", [(2, 4, 11), (1, 3, 17)])
def test_beam_slots_hold_the_kv_a_replay_writes(B, K, steps):
    from genvc_amd.engine import BeamSearch
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 29)
    eng = g.engine
    cond = synth.uniform(2950, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(2950, "content_codes", (B, 9), 256).to(DEV)
    fake = g.compute_embeddings(cond, codes)
    prefix = g._prefix
    n0 = int(fake.shape[1])
    slots = torch.arange(B * K, device=DEV, dtype=torch.int32)
    eng.prefill(slots[::K].contiguous(), prefix, want_outputs=False)
    beam = BeamSearch(fake, K, 40, EOS, V, 1.0, 2.0, "4.33")
    eng.beam_generate(slots, beam, 1)                      # step 0: every child has parent 0 -- K-1 copies of one slot
    assert int(beam.n_copies[0]) == K - 1
    eng.beam_generate(slots, beam, steps - 1)
    torch.cuda.synchronize()
    eng.health()
    T = beam.steps
    toks = beam.ids[T & 1, :, n0:n0 + T].clone()
    spare = torch.tensor([B * K], device=DEV, dtype=torch.int32)
    probe = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    for r in range(B * K):
        b = r // K
        eng.reset(spare)
        eng.prefill(spare, prefix[b:b + 1].contiguous(), want_outputs=False)
        for j in range(T):
            eng.decode_step(spare, toks[r, j:j + 1].contiguous())
        ref, _ = eng.decode_step(spare, probe)
        got, _ = eng.decode_step(slots[r:r + 1].contiguous(), probe)
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


# ---- 4. GenVCModel.inference(num_beams=4) --------------------------------------------------------------------------------------
def test_model_inference_with_beams():
    from chain_oracle import synthetic_bundle
    from genvc_amd.inference.model_init import model_init_synthetic
    from oracle import genvc_oracle as O
    cfg = gcfg.default_config(tiny=True)
    m = model_init_synthetic(cfg, seed=1, device=DEV, max_slots=8)[0]
    m.gpt.max_gen_mel_tokens = 30
    src = synth.uniform(402, "src_wav", (1, 16000), 0.3).to(DEV)
    ref = synth.uniform(100, "ref_wav", (1, 24000 * 3), 0.3).to(DEV)
    cond = m.get_gpt_cond_latents(ref, 24000)
    kw = dict(do_sample=False, num_beams=4, repetition_penalty=2.0, length_penalty=1.0)
    wav = m.inference(src, cond, **kw)
    feat = m.content_extractor.extract_content_features(src)
    codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
    gen = m.gpt.generate(cond, codes, **kw)[0]
    gen = gen[gen != EOS]
    assert gen.numel() > 0 and wav.shape[-1] == gen.numel() * 4 * 256
    W = synthetic_bundle(cfg, 1, 30)
    lat = O.gpt_latents(W["gpt"], W["dims"], cond.cpu(), codes.cpu().long(), gen.cpu().unsqueeze(0))
    want = O.vocode_latents(W["hifigan"], W["vocoder_cfg"], lat)
    torch.testing.assert_close(wav.cpu().reshape(-1), want.reshape(-1), rtol=2e-3, atol=2e-3)


# ---- 5. num_beams = 1 is unchanged; warmed-up beam calls do not allocate ---------------------------------------------------------
def test_num_beams_1_unchanged_and_beam_path_warm():
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 29)
    eng = g.engine
    g.max_gen_mel_tokens = 24
    cond = synth.uniform(2950, "cond_latents", (2, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(2950, "content_codes", (2, 9), 256).to(DEV)
    greedy = dict(top_k=1, repetition_penalty=2.0)
    n0 = 32 + 9 + 3
    eng.warmup(2, n0 + 24, 1)
    eng.warmup_range(2, n0 + 1, n0 + 24, 1)
    eng.warmup_beam(2, 4, n0 + 24)
    a = g.generate(cond, codes, **greedy)
    v = eng.decode_variant()
    base = eng.lazy_inits()
    b = g.generate(cond, codes, num_beams=1, **greedy)
    assert torch.equal(a, b) and eng.decode_variant() == v
    assert eng.lazy_inits() == base
    g.generate(cond, codes, num_beams=4, do_sample=False, repetition_penalty=2.0)
    assert eng.lazy_inits() == base                       # the warmed beam path neither allocates nor captures
