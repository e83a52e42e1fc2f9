"""GPU: num_return_sequences for GPT.generate -- the KV fan-out (include/genvc_hip.h: gvc_gpt_kv_fanout), N sampled candidates from one
prefill, their score (gvc_gpt_sequence_logprobs), N-best beam search and early_stopping against tests/golden/nbest.npz (the reference's
GPT.generate executed, scripts/make_nbest_golden.py) and the CPU restatement (tests/nbest_oracle.py), and the upper layers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402
import nbest_oracle as NO                     # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "nbest.npz")
EOS = 1025
GREEDY = dict(gcfg.DEFAULT_SAMPLING, top_k=1)


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


def close(g):
    g.engine.close()
    del g
    torch.cuda.empty_cache()


def inputs(seed, dims, B, Tc):
    cond = synth.uniform(seed, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(seed, "content_codes", (B, Tc), 256).to(DEV)
    return cond, codes


# ---- 1. beam fixtures: N-best and early_stopping ---------------------------------------------------------------------------------
def beam_case(gold, tag, **kw):
    margs = gcfg.DEFAULT_MODEL_ARGS if int(gold[f"{tag}_full"]) else gcfg.TINY_MODEL_ARGS
    sb = float(gold[f"{tag}_stop_bias"])
    g, w, dims = make_gpt(margs, int(gold[f"{tag}_seed"]), stop_bias=sb if sb != 0.0 else None, **kw)
    g.max_gen_mel_tokens = int(gold[f"{tag}_max_new"])
    cond, codes = inputs(int(gold[f"{tag}_in_seed"]), dims, int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]))
    return g, w, dims, cond, codes


@pytest.mark.parametrize("rows_step", ["1", "0"])
@pytest.mark.parametrize("tag", NO.TAGS)
def test_beam_fixture_cases_bit_for_bit(tag, rows_step, monkeypatch):
    """every fixture case (ids, order, width) through GPT.generate in mode "generated", on both decode classes; last_beam_scores
    against the restatement within the tolerance tests/test_gpu_beam.py uses for scores (rtol 1e-4)"""
    monkeypatch.setenv("GVC_PERSIST_ROWS", rows_step)
    gold = dict(np.load(GOLD))
    g, w, dims, cond, codes = beam_case(gold, tag)
    ora = BO.OracleGpt(w, dims)
    K, rep, max_new = int(gold[f"{tag}_K"]), float(gold[f"{tag}_rep"]), int(gold[f"{tag}_max_new"])
    for i in range(int(gold[f"{tag}_n"])):
        p = f"{tag}_{i}_"
        N, lp, early = int(gold[p + "N"]), float(gold[p + "lp"]), NO.EARLY[int(gold[p + "early"])]
        assert float(gold[p + "min_gap"]) >= 1e-3 and float(gold[p + "order_gap"]) >= 1e-3          # the margin screens
        ids = g.generate(cond, codes.long(), num_beams=K, do_sample=False, length_penalty=lp, repetition_penalty=rep,
                         num_return_sequences=N, early_stopping=early, beam_length_mode="generated", group=8)
        assert np.array_equal(ids.cpu().numpy(), gold[p + "ids"]), (tag, i, N, lp, early)
        r = NO.beam_search(ora, cond.cpu(), codes.cpu(), K, lp, rep, max_new, mode="generated", early_stopping=early, num_return=N)
        assert g.last_beam_scores.shape == (ids.shape[0],)
        np.testing.assert_allclose(g.last_beam_scores.numpy(), r["scores"], rtol=1e-4)
    close(g)


def test_one_return_with_early_stopping_false_is_todays_path():
    """N = 1, early_stopping=False: the kwargs given explicitly change nothing, bit for bit (ids and score)"""
    gold = dict(np.load(GOLD))
    tag = NO.TAGS[0]
    g, _, _, cond, codes = beam_case(gold, tag)
    kw = dict(num_beams=int(gold[f"{tag}_K"]), do_sample=False, repetition_penalty=float(gold[f"{tag}_rep"]), length_penalty=1.0)
    for mode in ("4.33", "generated"):
        a = g.generate(cond, codes, beam_length_mode=mode, **kw)
        sa = g.last_beam_scores.clone()
        b = g.generate(cond, codes, beam_length_mode=mode, num_return_sequences=1, early_stopping=False, **kw)
        assert torch.equal(a, b) and torch.equal(sa, g.last_beam_scores)
    close(g)


@pytest.mark.parametrize("early", [False, True, "never"])
@pytest.mark.parametrize("mode", ["4.33", "generated"])
@pytest.mark.parametrize("B,K", [(3, 4), (1, 8), (3, 2)])
def test_select_step_matches_restatement_step_by_step(B, K, mode, early):
    """the device select step against the restatement step by step on random logits, as tests/test_gpu_beam.py does for
    early_stopping=False (mode "4.33" has no executed reference here: its generation code is not installed): tokens, parents,
    running scores, the done flags -- the early_stopping test -- and the kept hypotheses; then the N-best finalisation"""
    from genvc_amd.engine import BeamSearch, beam_select
    V = 1026
    n0, max_new, rep = 7, 12, 2.0
    # (seeds screened with the restatement alone: every gap of every step and every pair of kept scores >= 5e-5 in all six mode pairs)
    gen_ = torch.Generator().manual_seed({(3, 4): 1, (1, 8): 113, (3, 2): 2}[(B, K)] + 1000 * B + K)
    fake = torch.randint(0, 1024, (B, n0), generator=gen_)
    fake[:, -1] = 1024
    done_at = set()
    for lp in (0.5, 1.0, 2.0):
        beam = BeamSearch(fake.to(DEV), K, max_new, EOS, V, lp, rep, mode, early_stopping=early)
        slots = torch.arange(B * K, device=DEV, dtype=torch.int32)
        scores = beam.scores.cpu().clone()
        gen = [[] for _ in range(B * K)]
        hyps = [BO.Hyps(K) for _ in range(B)]
        done = [False] * B
        ids = fake.repeat_interleave(K, 0)
        T = 0
        for t in range(max_new):
            logits = torch.randn(B * K, V, generator=gen_) * 3.0
            logits[:, EOS] += float([9.0, 3.0, 5.0, 1.0, 7.0, 4.0][t % 6])
            s = BO.log_probs(logits, ids, rep)
            tok, par, scores, gen, gap = NO.select_step(s, scores, gen, hyps, done, t, n0, K, V, EOS, lp, mode, early, max_new)
            assert gap > 1e-5, f"near-tie in the random case (gap {gap:.2e}): pick another seed"
            beam_select(beam, logits.to(DEV).contiguous(), slots, t)
            beam.steps = T = t + 1
            torch.cuda.synchronize()
            assert np.array_equal(beam.tokens.cpu().numpy(), tok.numpy()), (t, lp)
            assert np.array_equal(beam.parents.cpu().numpy(), par.numpy()), (t, lp)
            torch.testing.assert_close(beam.scores.cpu(), scores.float(), rtol=1e-5, atol=1e-4)
            assert beam.done.cpu().tolist() == [int(x) for x in done], (t, lp, early)
            assert beam.hyp_count.cpu().tolist() == [len(h.items) for h in hyps], (t, lp)
            src = (torch.arange(B).repeat_interleave(K) * K + par).long()
            ids = torch.cat([ids[src], tok[:, None]], 1)
            done_at.update((lp, b, t) for b in range(B) if done[b])
            if all(done):
                break
        for N in (1, K):
            hy = [BO.Hyps(K) for _ in range(B)]
            for h, src_h in zip(hy, hyps):
                h.items, h.worst = list(src_h.items), src_h.worst
            want, wsc, og = NO.finalize(hy, done, scores, gen, n0, T, K, EOS, lp, mode, max_new, N)
            assert og > 1e-5
            got, gsc = beam.finalize(N)
            assert np.array_equal(got.cpu().numpy(), want), (lp, N)
            np.testing.assert_allclose(gsc.numpy(), wsc, rtol=1e-4, atol=1e-5)
    assert done_at                       # some item was done before the budget: the test under `early` decided something


# ---- 2. the fan-out -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_step", ["1", "0"])
@pytest.mark.parametrize("name,margs", [("gpt_tiny_b1", gcfg.TINY_MODEL_ARGS), ("gpt_full", gcfg.DEFAULT_MODEL_ARGS)], ids=["tiny", "full"])
def test_fanned_out_rows_reproduce_the_greedy_fixture(gold, name, margs, rows_step, monkeypatch):
    """do_sample=True, top_k=1, num_return_sequences=4 on the margin-screened greedy fixtures: every candidate row decodes from the
    fanned-out copy of the one prefilled slot, so all four must be the reference's greedy ids (a wrong or short KV copy, a missing
    length / mel position or a stale parked logits row breaks this)"""
    monkeypatch.setenv("GVC_PERSIST_ROWS", rows_step)
    gd = gold(name)
    g, _, dims = make_gpt(margs, int(gd["seed"]), max_slots=8)
    cond, codes = inputs(int(gd["in_seed"]), dims, int(gd["B"]), int(gd["Tc"]))
    n = gd["tokens"].shape[1]
    ids = g.generate(cond, codes, do_sample=True, num_return_sequences=4, max_new_tokens=n, **GREEDY)
    assert ids.shape == (4 * int(gd["B"]), n)
    for j in range(4):
        assert np.array_equal(ids[j::4].cpu().numpy(), gd["tokens"]), j
    close(g)


@pytest.mark.parametrize("wd", ["fp32", "bf16_kv"])
@pytest.mark.parametrize("margs,B,N,Tc", [(gcfg.TINY_MODEL_ARGS, 2, 3, 11), (gcfg.DEFAULT_MODEL_ARGS, 1, 4, 13)], ids=["tiny", "full"])
def test_fanout_equals_single_item_prefills(margs, B, N, Tc, wd):
    """run A prefills item b into slot b*N with a single-item prefill and fans it out; run B prefills each of the B*N slots with the
    same single-item prefill call (the same kernel class on both sides: a B*N-row batched prefill may sum in another order).  Both
    then go through the same B*N-row sampled decode with the same seed: tokens and latents bit-identical, fp32 and bf16 KV"""
    from genvc_amd.engine import sample_params
    g, _, dims = make_gpt(margs, 7, max_slots=8, weight_dtype=wd)
    eng = g.engine
    cond, codes = inputs(701, dims, B, Tc)
    prefix = eng.prefix_embeddings(cond, codes.int())
    P, steps = prefix.shape[1], 24
    slots = torch.arange(B * N, device=DEV, dtype=torch.int32)
    samp = dict(repetition_penalty=2.0, temperature=1.0, top_p=1.0, top_k=50)

    def decode():
        ids = torch.ones(B * N, P + 1 + steps + 8, device=DEV, dtype=torch.int32)
        ids[:, P] = dims["start_audio_token"]
        ids_len = torch.full((B * N,), P + 1, device=DEV, dtype=torch.int32)
        fin = torch.zeros(B * N, device=DEV, dtype=torch.int32)
        toks = torch.full((B * N, steps), -1, device=DEV, dtype=torch.int32)
        lats = torch.zeros(B * N, steps, dims["d_model"], device=DEV)
        sp = sample_params(samp, dims["num_audio_tokens"], EOS, 5)
        eng.generate(slots, ids, ids_len, fin, sp, 0, 8, toks, lats, max_keys=P + 1 + steps)
        eng.generate(slots, ids, ids_len, fin, sp, 8, steps - 8, toks, lats, max_keys=P + 1 + steps)
        torch.cuda.synchronize()
        eng.health()
        return toks.cpu(), lats.cpu()

    for b in range(B):
        eng.prefill(slots[b * N:b * N + 1].contiguous(), prefix[b:b + 1].contiguous(), want_outputs=False)
    src = slots[::N].contiguous().repeat_interleave(N - 1)
    dst = slots.view(B, N)[:, 1:].reshape(-1).contiguous()
    eng.kv_fanout(src, dst)
    ta, la = decode()
    eng.reset(slots)
    for r in range(B * N):
        eng.prefill(slots[r:r + 1].contiguous(), prefix[r // N:r // N + 1].contiguous(), want_outputs=False)
    tb, lb = decode()
    assert torch.equal(ta, tb) and torch.equal(la, lb)
    # the decode sampled: the candidates of an item differ somewhere (top_k 50, temperature 1)
    assert any(not torch.equal(ta[b * N], ta[b * N + j]) for b in range(B) for j in range(1, N))
    close(g)


def test_fanout_skips_bad_pairs_and_checks_its_arguments():
    from genvc_amd._lib import GenvcHipError
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 7, max_slots=4)
    eng = g.engine
    cond, codes = inputs(701, dims, 1, 9)
    prefix = eng.prefix_embeddings(cond, codes.int())
    s0 = torch.zeros(1, device=DEV, dtype=torch.int32)
    eng.prefill(s0, prefix, want_outputs=False)
    probe = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    # slots outside the context and src == dst copy nothing (and write nothing out of bounds)
    eng.kv_fanout(torch.tensor([0, 0, 9, 0], device=DEV, dtype=torch.int32), torch.tensor([4, -1, 1, 0], device=DEV, dtype=torch.int32))
    eng.kv_fanout(s0, torch.tensor([2], device=DEV, dtype=torch.int32))
    a, _ = eng.decode_step(s0, probe)
    b, _ = eng.decode_step(torch.tensor([2], device=DEV, dtype=torch.int32), probe)
    assert torch.equal(a, b)
    with pytest.raises(ValueError):
        eng.kv_fanout(s0, torch.zeros(2, device=DEV, dtype=torch.int32))
    with pytest.raises(GenvcHipError):
        eng.kv_fanout(torch.zeros(5, device=DEV, dtype=torch.int32), torch.ones(5, device=DEV, dtype=torch.int32))      # n > max_slots
    close(g)


# ---- 3. the sampled call ---------------------------------------------------------------------------------------------------------
def test_sampled_call_shape_order_and_expansion():
    """[B*N, n] rows ordered b*N + j; at top_k=50, temperature=1 the N rows of an item are not all equal; the call equals generate on
    repeat_interleave(N) inputs -- at this shape (tiny, 44-row prompts: 88 and 264 rows against 44 and 132) both prefills run on
    the skinny row GEMMs, whose rows do not depend on the row count, so the expanded call draws from the same logits.  Where the
    expanded prefill lands on the tiled GEMM instead (more than 128 rows) its sums may differ in the last bits and only
    test_fanout_equals_single_item_prefills applies.  The shape assertion fails without the feature (the kwarg was dropped: B rows)."""
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 43, stop_bias=2.0, max_slots=8)
    g.max_gen_mel_tokens = 24
    kw = dict(do_sample=True, top_k=50, temperature=1.0, top_p=1.0, repetition_penalty=2.0, seed=9)
    for B, N in ((1, 2), (2, 2)):
        cond, codes = inputs(4300, dims, B, 9)
        ids = g.generate(cond, codes, num_return_sequences=N, **kw)
        assert ids.dtype == torch.int64 and ids.shape[0] == B * N
        n = ids.shape[1]
        assert g.last_latents.shape == (B * N, n, dims["d_model"])
        assert g.last_sequence_logprobs.shape == (B * N,) and g.last_sequence_logprobs.dtype == torch.float64
        assert g.last_sequence_lengths.shape == (B * N,) and g.last_sequence_lengths.dtype == torch.int64
        for b in range(B):
            assert any(not torch.equal(ids[b * N], ids[b * N + j]) for j in range(1, N)), b
        exp = g.generate(cond.repeat_interleave(N, 0), codes.repeat_interleave(N, 0), **kw)
        assert torch.equal(ids, exp), (B, N)
        # N = 1 is the call without the kwarg
        one = g.generate(cond, codes, **kw)
        assert torch.equal(one, g.generate(cond, codes, num_return_sequences=1, **kw)) and one.shape[0] == B
        assert g.last_sequence_logprobs is None
    close(g)


def test_refused_and_bounded_calls():
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 43, max_slots=8)
    g.max_gen_mel_tokens = 8
    cond, codes = inputs(4300, dims, 3, 9)
    with pytest.raises(ValueError, match="KV slots"):
        g.generate(cond, codes, do_sample=True, num_return_sequences=3)                       # 3 x 3 > 8 slots
    with pytest.raises(ValueError, match="greedy"):
        g.generate(cond, codes, do_sample=False, num_return_sequences=2)
    with pytest.raises(ValueError, match="at least 1"):
        g.generate(cond, codes, do_sample=True, num_return_sequences=0)
    with pytest.raises(NotImplementedError, match="get_generator"):
        next(g.get_generator(g.compute_embeddings(cond, codes), num_return_sequences=2))
    with pytest.raises(NotImplementedError, match="generate_groups"):
        g.generate_groups([(cond, codes)], num_return_sequences=2)
    with pytest.raises(NotImplementedError, match="generate_rolling"):
        g.generate_rolling([(cond, codes)], num_return_sequences=2)
    assert g.generate(cond, codes, do_sample=True, num_return_sequences=2, top_k=5).shape[0] == 6      # 3 x 2 fits
    close(g)


# ---- 4. sequence_logprobs ---------------------------------------------------------------------------------------------------------
def ref_logprobs(w, tokens, latents, dtype):
    """(per-token log-probabilities [R, n], lengths [R]) of the same computation in torch on the CPU at `dtype`"""
    W, b = w["mel_head.weight"].to(dtype), w["mel_head.bias"].to(dtype)
    lp = torch.log_softmax(latents.to(dtype) @ W.T + b, -1).gather(-1, tokens.long().unsqueeze(-1)).squeeze(-1)
    R, n = tokens.shape
    stop = tokens == EOS
    lens = torch.where(stop.any(1), stop.int().argmax(1) + 1, torch.full((R,), n))
    return lp, lens


@pytest.mark.parametrize("margs", [gcfg.TINY_MODEL_ARGS, gcfg.DEFAULT_MODEL_ARGS], ids=["tiny", "full"])
def test_sequence_logprobs_within_the_fp32_yardstick(margs):
    """against float64 from the same downloaded latents and the bound weights, by the first term of tests/act_stats.py::yardstick:
    per token the deviation is at most 8x that of the same computation in fp32 torch on the CPU + 1e-6 max|ref|; the per-sequence
    sum stays within that bound times the length.  Prints the three numbers."""
    g, w, dims = make_gpt(margs, 43, stop_bias=1.0, max_slots=8)
    g.max_gen_mel_tokens = 60
    cond, codes = inputs(4300, dims, 2, 13)
    ids = g.generate(cond, codes, do_sample=True, top_k=50, temperature=1.0, repetition_penalty=2.0, seed=3, num_return_sequences=4)
    lats = g.last_latents
    lp, ln, tl = g.engine.sequence_logprobs(ids.int(), lats, token_logprobs=True)
    assert torch.equal(lp, g.last_sequence_logprobs) and torch.equal(ln.long(), g.last_sequence_lengths)
    wc = {k: torch.as_tensor(v).cpu() for k, v in w.items()}
    r64, lens = ref_logprobs(wc, ids.cpu(), lats.cpu(), torch.float64)
    r32, _ = ref_logprobs(wc, ids.cpu(), lats.cpu(), torch.float32)
    assert torch.equal(ln.cpu().long(), lens)
    mask = torch.arange(ids.shape[1])[None, :] < lens[:, None]
    dk = float(((tl.cpu().double() - r64).abs() * mask).max())
    d32 = float(((r32.double() - r64).abs() * mask).max())
    bound = 8.0 * d32 + 1e-6 * float((r64 * mask).abs().max())
    print(f"sequence_logprobs {margs['gpt_n_model_channels']}: kernel {dk:.3e}  fp32 torch {d32:.3e}  bound {bound:.3e}")
    assert dk <= bound
    assert float((tl.cpu() * ~mask).abs().max()) == 0.0                      # nothing past a row's length
    dsum = (lp.cpu() - (r64 * mask).sum(1)).abs()
    print(f"  per-sequence sums: worst {float(dsum.max()):.3e} over lengths {lens.tolist()}")
    assert bool((dsum <= bound * lens.double()).all())
    close(g)


def test_sequence_logprobs_edge_cases():
    """rows ending at different steps, a row without a stop token, a row whose first token is the stop token, tokens wider than any
    row and than the latents; a sequence count above one scratch chunk is not needed for these"""
    g, w, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 43, max_slots=4)
    gen = torch.Generator().manual_seed(5)
    R, n, d = 4, 12, dims["d_model"]
    lats = torch.randn(R, n, d, generator=gen)
    toks = torch.randint(0, 1024, (R, n + 5), generator=gen)
    toks[0, 4] = EOS
    toks[0, 7] = EOS                 # only the first stop token counts
    toks[2, 0] = EOS
    toks[3, n - 1] = EOS
    toks[:, n:] = EOS                # the columns past the latents are not looked at (row 1 has no stop token within n)
    lp, ln = g.sequence_logprobs(toks.to(DEV), lats.to(DEV))
    assert lp.dtype == torch.float64 and ln.dtype == torch.int64
    wc = {k: torch.as_tensor(v).cpu() for k, v in w.items()}
    r64, lens = ref_logprobs(wc, toks[:, :n], lats, torch.float64)
    assert lens.tolist() == [5, n, 1, n] and ln.cpu().tolist() == lens.tolist()
    mask = torch.arange(n)[None, :] < lens[:, None]
    np.testing.assert_allclose(lp.cpu().numpy(), (r64 * mask).sum(1).numpy(), rtol=0, atol=1e-4)
    with pytest.raises(ValueError):
        g.engine.sequence_logprobs(toks[:, :n - 1].int().to(DEV), lats.to(DEV))               # fewer tokens than latent rows
    close(g)


def test_sequence_logprobs_over_several_scratch_chunks():
    """R * n * vocab above half the context's scratch (4M floats): the head GEMM and the row kernel run once per chunk of whole
    sequences, offsetting tokens, sums, lengths and per-token terms by the chunk's first row.  R = 64, n = 80: 5.25M logits, two chunks"""
    g, w, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 43, max_slots=4)
    gen = torch.Generator().manual_seed(6)
    R, n, d = 64, 80, dims["d_model"]
    assert R * n * dims["num_audio_tokens"] > 4 << 20 and n * dims["num_audio_tokens"] < 4 << 20
    lats = torch.randn(R, n, d, generator=gen)
    toks = torch.randint(0, 1024, (R, n), generator=gen)
    for r in range(R):
        if r % 3:
            toks[r, (7 * r) % n] = EOS               # ragged ends on both sides of the chunk boundary; every third row has no stop token
    lp, ln, tl = g.engine.sequence_logprobs(toks.int().to(DEV), lats.to(DEV), token_logprobs=True)
    wc = {k: torch.as_tensor(v).cpu() for k, v in w.items()}
    r64, lens = ref_logprobs(wc, toks, lats, torch.float64)
    assert ln.cpu().tolist() == lens.tolist() and len(set(lens.tolist())) > 10
    mask = torch.arange(n)[None, :] < lens[:, None]
    np.testing.assert_allclose(tl.cpu().double().numpy(), (r64 * mask).numpy(), rtol=0, atol=1e-4)
    np.testing.assert_allclose(lp.cpu().numpy(), (r64 * mask).sum(1).numpy(), rtol=0, atol=1e-4 * n)
    close(g)


def test_sequence_logprobs_with_bf16_weights_scores_the_rounded_head():
    """bf16 weight storage: the context keeps mel_head rounded to bf16 in BOTH its copies (the fp32 array the score's GEMM reads holds
    the rounded values), so the score is that of the head the loop drew from.  Same yardstick as at fp32, the float64 / fp32 references
    computed with the weights rounded the same way"""
    g, w, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 43, stop_bias=1.0, max_slots=8, weight_dtype="bf16")
    g.max_gen_mel_tokens = 40
    cond, codes = inputs(4300, dims, 2, 13)
    ids = g.generate(cond, codes, do_sample=True, top_k=50, temperature=1.0, repetition_penalty=2.0, seed=3, num_return_sequences=3)
    lats = g.last_latents
    lp, ln, tl = g.engine.sequence_logprobs(ids.int(), lats, token_logprobs=True)
    wc = {"mel_head.weight": torch.as_tensor(w["mel_head.weight"]).cpu().to(torch.bfloat16).float(),
          "mel_head.bias": torch.as_tensor(w["mel_head.bias"]).cpu()}
    r64, lens = ref_logprobs(wc, ids.cpu(), lats.cpu(), torch.float64)
    r32, _ = ref_logprobs(wc, ids.cpu(), lats.cpu(), torch.float32)
    assert torch.equal(ln.cpu().long(), lens)
    mask = torch.arange(ids.shape[1])[None, :] < lens[:, None]
    dk = float(((tl.cpu().double() - r64).abs() * mask).max())
    d32 = float(((r32.double() - r64).abs() * mask).max())
    bound = 8.0 * d32 + 1e-6 * float((r64 * mask).abs().max())
    print(f"sequence_logprobs bf16 weights: kernel {dk:.3e}  fp32 torch {d32:.3e}  bound {bound:.3e}")
    assert dk <= bound
    close(g)


def test_fanout_call_honours_cached_cond_rows_and_retries_over_all_slots(monkeypatch):
    """cached_cond_rows: the one prefilled slot of an item keeps its conditioning rows from the previous call, the call's ids do not
    change.  A hand-off time-out (simulated: the first decode group raises the library's time-out error) resets all B*N slots and
    repeats from a full prefill"""
    from genvc_amd._lib import GVC_ERR_TIMEOUT, GenvcHipError
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 43, stop_bias=2.0, max_slots=8)
    g.max_gen_mel_tokens = 20
    B, N = 2, 3
    cond, codes = inputs(4300, dims, B, 9)
    kw = dict(do_sample=True, top_k=50, temperature=1.0, repetition_penalty=2.0, seed=9, num_return_sequences=N)
    want = g.generate(cond, codes, **kw)
    prefills = []
    real_prefill = g.engine.prefill
    monkeypatch.setattr(g.engine, "prefill", lambda slots, *a, **k: (prefills.append((slots.cpu().tolist(), k.get("n_cached", 0))),
                                                                      real_prefill(slots, *a, **k))[1])
    got = g.generate(cond, codes, cached_cond_rows=32, **kw)            # (slots 0 and N still hold this speaker's conditioning rows)
    assert torch.equal(got, want) and prefills == [([0, N], 32)]
    resets, fails = [], [1]
    real_reset, real_advance = g.engine.reset, g._advance
    monkeypatch.setattr(g.engine, "reset", lambda slots: (resets.append(slots.cpu().tolist()), real_reset(slots))[1])

    def advance(st, n):
        if fails:
            fails.pop()
            raise GenvcHipError("simulated hand-off time-out", GVC_ERR_TIMEOUT)
        return real_advance(st, n)
    monkeypatch.setattr(g, "_advance", advance)
    del prefills[:]
    base = g.recoveries
    got = g.generate(cond, codes, cached_cond_rows=32, **kw)
    assert torch.equal(got, want) and g.recoveries == base + 1
    assert resets == [list(range(B * N))]
    assert prefills == [([0, N], 32), ([0, N], 0)]                       # the retry prefills in full: the reset slots lost their rows
    close(g)


# ---- 5. GenVCModel.inference, warm-up, the CLI -----------------------------------------------------------------------------------
def tiny_model(max_slots=8):
    from genvc_amd.inference.model_init import model_init_synthetic
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=1, device=DEV, max_slots=max_slots)[0]
    m.gpt.max_gen_mel_tokens = 30
    return m


def test_model_inference_returns_n_waveforms_and_stays_warm():
    m = tiny_model()
    src = synth.uniform(402, "src_wav", (1, 16000), 0.3).to(DEV)
    ref = synth.uniform(100, "ref_wav", (1, 24000 * 3), 0.3).to(DEV)
    cond = m.get_gpt_cond_latents(ref, 24000)
    N = 3
    m.warmup(seg_len=1.0, streams=1, ref_seconds=3.0, max_new_tokens=30, num_return_sequences=N)
    feat = m.content_extractor.extract_content_features(src)
    codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
    base = m.gpt.engine.lazy_inits()
    wavs = m.inference(src, cond, generate_kwargs={"num_return_sequences": N, "seed": 4})
    assert m.gpt.engine.lazy_inits() == base                  # neither an allocation nor a capture inside the N-return call
    rows = m.gpt.generate(cond, codes, do_sample=True, top_p=0.85, top_k=15, temperature=0.75, repetition_penalty=10.0,
                          num_return_sequences=N, seed=4)
    assert isinstance(wavs, list) and len(wavs) == N and rows.shape[0] == N
    for j in range(N):
        assert wavs[j].shape[-1] == int((rows[j] != EOS).sum()) * 1024, j
    assert m.last_sequence_logprobs.shape == (N,)
    assert torch.equal(m.last_sequence_logprobs, m.gpt.last_sequence_logprobs)
    same = m.inference(src, cond, num_return_sequences=N, generate_kwargs={"seed": 4})
    assert all(torch.equal(a, b) for a, b in zip(wavs, same))
    # N = 1: the waveform of the call without the kwarg, not a list
    one = m.inference(src, cond, generate_kwargs={"seed": 4})
    again = m.inference(src, cond, generate_kwargs={"seed": 4, "num_return_sequences": 1})
    assert torch.is_tensor(again) and torch.equal(one, again)
    # the N best beams: the re-pass latents, the beam scores
    bw = m.inference(src, cond, do_sample=False, num_beams=3, generate_kwargs={"num_return_sequences": 2})
    brows = m.gpt.generate(cond, codes, do_sample=False, num_beams=3, num_return_sequences=2, repetition_penalty=10.0)
    assert len(bw) == 2 and m.gpt.last_beam_scores.shape == (2,)
    for j in range(2):
        assert bw[j].shape[-1] == int((brows[j] != EOS).sum()) * 1024
    from genvc_amd.streaming import StreamSessions
    with pytest.raises(NotImplementedError, match="StreamSessions"):
        StreamSessions(m, generate_kwargs={"num_return_sequences": 2})
    from genvc_amd.inference.inference_utils import synthesize_utt_chunked
    with pytest.raises(NotImplementedError, match="synthesize_utt_chunked"):
        synthesize_utt_chunked(m, src, ref, generate_kwargs={"num_return_sequences": 2})


def test_cli_writes_one_file_per_candidate(tmp_path):
    import wave
    from genvc_amd.audio import save_wav
    src = synth.uniform(402, "src_wav", (16000,), 0.3)
    ref = synth.uniform(100, "ref_wav", (24000 * 3,), 0.3)
    save_wav(str(tmp_path / "src.wav"), src, 16000)
    save_wav(str(tmp_path / "ref.wav"), ref, 24000)
    out = tmp_path / "out.wav"
    tok = tmp_path / "tok.pt"
    cmd = [sys.executable, os.path.join(ROOT, "infer.py"), "--synthetic", "--tiny", "--src_wav", str(tmp_path / "src.wav"),
           "--ref_audio", str(tmp_path / "ref.wav"), "--output_path", str(out), "--num_return_sequences", "3", "--seg_len", "1.0",
           "--save_tokens", str(tok)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    saved = torch.load(str(tok))
    assert len(saved) == 3
    lines = [ln for ln in r.stdout.splitlines() if "log-probability" in ln]
    assert len(lines) == 3
    for j, s in enumerate(saved):
        n = 0 if s["tokens"] is None else int(s["tokens"].numel())
        assert f"out_{j}.wav: {n} codec tokens" in lines[j]
        if n:
            with wave.open(str(tmp_path / f"out_{j}.wav"), "rb") as f:
                assert f.getframerate() == 24000 and f.getnframes() == n * 1024      # (the vocoder's rate is the file's: factor 1)
    bad = subprocess.run(cmd + ["--streaming"], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert bad.returncode != 0 and "num_return_sequences" in bad.stderr
