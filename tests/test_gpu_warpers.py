"""GPU: the typical / epsilon / eta sampling warpers (include/genvc_hip.h: gvc_logits_warpers, gvc_sample_warp, gvc_gpt_generate_warp)
against tests/golden/logits_warpers.npz (the reference's sample_stream with the installed transformers' warpers, executed:
scripts/make_warper_golden.py) on every decode path, draws against HF's kept set and probabilities, the off / null / greedy / beam
invariants and the warm path."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_processors as TP              # noqa: E402
import warp_oracle as WO                      # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logits_warpers.npz")
EOS, V = 1025, 1026
OFF = dict(typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def cases(gold):
    return json.loads(str(gold["cases"]))


def load_case(gold, tag):
    """(GPT, cond, codes, warper kwargs, sampling kwargs) of a fixture case"""
    full = bool(gold[f"{tag}_full"])
    g, dims = TP.make_gpt(gcfg.DEFAULT_MODEL_ARGS if full else gcfg.TINY_MODEL_ARGS, int(gold[f"{tag}_seed"]))
    g.max_gen_mel_tokens = int(gold[f"{tag}_max_new"])
    B, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(s, "content_codes", (B, Tc), 256).to(DEV)
    return g, cond, codes, json.loads(str(gold[f"{tag}_kw"])), dict(json.loads(str(gold[f"{tag}_samp"])), do_sample=True)


def _stop_len(t):
    hit = t == EOS
    return t.shape[1] if not hit.any(1).all() else int(hit.argmax(1).max()) + 1


# ---- 1. GPT.generate: every case at B = 1 and at the fixture's B, on both decode classes ----------------------------------------
@pytest.mark.parametrize("one_launch", ["1", "0"], ids=["one_launch_steps", "launch_per_phase"])
def test_generate_matches_executed_reference(gold, one_launch, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST", one_launch)
    monkeypatch.setenv("GVC_PERSIST_ROWS", one_launch)
    for tag in cases(gold):
        g, cond, codes, kw, samp = load_case(gold, tag)
        want = gold[f"{tag}_tokens"]
        for seed in (0, 9):                               # one survivor per step: the key does not matter
            got = g.generate(cond, codes, group=8, seed=seed, **samp, **kw).cpu().numpy()
            assert np.array_equal(got, want), (tag, seed)
        one = g.generate(cond[:1], codes[:1], group=8, **samp, **kw).cpu().numpy()
        assert np.array_equal(one[0], TP.trim(want[0])), tag
        # without the warpers the call samples other ids
        assert not np.array_equal(g.generate(cond, codes, group=8, **samp).cpu().numpy(), want), tag
        TP._close(g)


# ---- 2. get_generator: streamed pairs, latents against the teacher-forced re-pass ----------------------------------------------
def test_get_generator_matches_executed_reference(gold):
    for tag in cases(gold):
        g, cond, codes, kw, samp = load_case(gold, tag)
        want = gold[f"{tag}_tokens"]
        fake = g.compute_embeddings(cond, codes)
        pairs = list(g.get_generator(fake_inputs=fake, stream_group=8, **samp, **kw))
        toks = torch.stack([p[0] for p in pairs], 1).cpu().numpy()
        lats = torch.stack([p[1] for p in pairs], 1)
        assert np.array_equal(toks, want), tag
        gen = torch.from_numpy(TP.trim(want[0]))
        gen = gen[gen != EOS].unsqueeze(0).to(DEV)
        Tc = codes.shape[1]
        rel = g(codes[:1], torch.tensor([Tc], device=DEV), gen, torch.tensor([gen.shape[1] * 1024], device=DEV),
                cond_latents=cond[:1], return_latent=True)
        np.testing.assert_allclose(rel[0].cpu().numpy(), lats[0, :gen.shape[1]].cpu().numpy(), atol=1e-4)
        TP._close(g)


# ---- 3. per-item warpers: joint groups, rolling jobs, sessions ------------------------------------------------------------------
def _tiny_pair(gold):
    """the two tiny cases that share weights and sampling settings (typical, epsilon): their inputs and expected ids"""
    a, b = "typical", "epsilon"
    g, ca, xa, ka, samp = load_case(gold, a)
    _, _, _, kb, sb = load_case(gold, b)
    assert sb == samp and int(gold[f"{a}_seed"]) == int(gold[f"{b}_seed"])
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    s = int(gold[f"{b}_in_seed"])
    cb = synth.uniform(s, "cond_latents", (int(gold[f"{b}_B"]), 32, dims["d_model"]), 1.0).to(DEV)
    xb = synth.integers(s, "content_codes", (int(gold[f"{b}_B"]), int(gold[f"{b}_Tc"])), 256).to(DEV)
    return g, samp, [(ca, xa, ka, gold[f"{a}_tokens"]), (cb, xb, kb, gold[f"{b}_tokens"])]


def test_groups_and_rolling_with_per_item_warpers(gold):
    g, samp, items = _tiny_pair(gold)
    groups = [(c, x) for c, x, _, _ in items]
    kws = [k for _, _, k, _ in items]
    g.groups_stats = {"joint": 0, "separate": 0}
    outs = g.generate_groups(groups, group_kwargs=kws, joint_sampling=True, class_seeds=[3, 4], group=8, **samp)
    assert g.groups_stats["joint"] == 1
    for o, (c, x, k, want) in zip(outs, items):
        assert np.array_equal(o.cpu().numpy(), want[:, :_stop_len(want)])
    # the serial schedule and the solo generate() calls agree
    ser = g.generate_groups(groups, group_kwargs=kws, class_seeds=[3, 4], group=8, **samp)
    for o, s, (c, x, k, _) in zip(ser, (3, 4), items):
        assert torch.equal(o, g.generate(c, x, seed=s, **samp, **k))
    # call-wide warpers on the joint schedule: every group gets its generate(**kwargs)
    outs = g.generate_groups(groups, joint_sampling=True, class_seeds=[3, 4], group=8, **samp, **kws[0])
    assert np.array_equal(outs[0].cpu().numpy(), items[0][3][:, :_stop_len(items[0][3])])
    assert torch.equal(outs[1], g.generate(items[1][0], items[1][1], seed=4, **samp, **kws[0]))
    # rolling with job seeds: rows of different jobs and warpers share the decode calls (three rows in flight)
    jobs = [groups[0], groups[1], (groups[0][0][1:], groups[0][1][1:]), (groups[1][0][:1], groups[1][1][:1])]
    jk = [kws[0], kws[1], kws[0], None]
    rolled = g.generate_rolling(jobs, job_seeds=[5, 6, 7, 8], job_kwargs=jk, group=8, max_rows=3, **samp)
    for (c, x), a, s, k in zip(jobs, rolled, (5, 6, 7, 8), jk):
        assert torch.equal(a, g.generate(c, x, seed=s, **samp, **(k or {})))
    assert np.array_equal(rolled[0].cpu().numpy(), items[0][3][:, :_stop_len(items[0][3])])
    rolled = g.generate_rolling(jobs[:2], job_seeds=[5, 6], group=8, **samp, **kws[1])          # call-wide
    assert np.array_equal(rolled[1].cpu().numpy(), items[1][3][:, :_stop_len(items[1][3])])
    with pytest.raises(ValueError, match="typical_p"):
        g.generate_groups(groups, group_kwargs=[dict(typical_p=-1.0), None], joint_sampling=True, **samp)
    del g.groups_stats
    TP._close(g)


def test_stream_sessions_per_session_warpers():
    """sessions with different warpers (and one without) each get the tokens and waveform of their solo synthesize_utt_streaming"""
    from genvc_amd.inference.inference_utils import segments, synthesize_utt_streaming
    from genvc_amd.inference.model_init import model_init_synthetic
    from genvc_amd.streaming import StreamSessions
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=8)[0]
    m.gpt.max_gen_mel_tokens = 30
    cfg = m.config
    saved = dict(top_k=cfg.top_k, top_p=cfg.top_p, temperature=cfg.temperature, repetition_penalty=cfg.repetition_penalty)
    refs = [synth.synth_audio(60 + i, "ref", 72000) for i in range(3)]
    srcs = [synth.synth_audio(80 + i, "src", n) for i, n in enumerate((32000, 16000, 24000))]
    segs = [list(segments(s, 16000, 5120)) for s in srcs]
    setting = dict(top_k=20, top_p=1.0, temperature=0.3, repetition_penalty=2.0)
    seeds = [3, 4, 5]
    warps = [dict(typical_p=0.05), dict(epsilon_cutoff=0.25, eta_cutoff=0.5), None]

    def solo(i, gk):
        for k, v in dict(saved, **setting).items():
            setattr(cfg, k, v)
        try:
            r = synthesize_utt_streaming(m, srcs[i], refs[i], seg_len=1.0, stream_chunk_size=8, verbose=False, return_details=True,
                                         generate_kwargs=dict(gk or {}, seed=seeds[i]))
        finally:
            for k, v in saved.items():
                setattr(cfg, k, v)
        return torch.cat(r["tokens"], 1)[0].cpu(), r["wav"].cpu()

    ss = StreamSessions(m, max_sessions=3, group=8, per_session_sampling=True)
    sids, wavs = {}, {}
    for i in range(3):
        sids[i] = ss.open(refs[i], sampling=setting, seed=seeds[i], generate_kwargs=warps[i])
        for sg in segs[i]:
            ss.push(sids[i], sg)
    steps = 0
    while True:
        for sid, chunks in ss.step().items():
            wavs.setdefault(sid, []).extend(chunks)
        steps += 1
        if ss.idle():
            break
        assert steps < 200
    for i in range(3):
        toks, wav = solo(i, warps[i])
        got = torch.cat(ss.close(sids[i]), 1)[0].cpu()
        assert torch.equal(got, toks), f"session {i}: tokens differ from its solo run"
        np.testing.assert_allclose(torch.cat(wavs[sids[i]], -1).cpu().numpy(), wav.numpy(), atol=2e-4)
        if warps[i] is not None:
            assert not torch.equal(toks, solo(i, None)[0]), f"session {i}: its warpers change nothing"
    with pytest.raises(ValueError, match="not a processor kwarg"):
        ss.open(refs[0], generate_kwargs=dict(top_k=3))
    del m
    torch.cuda.empty_cache()


# ---- 4. draws through the sampler entry point against HF's kept set and probabilities -----------------------------------------
def _hf_probs(s, temperature, top_k, top_p, min_p, kw):
    from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    x = s[None].clone()
    warpers = [TemperatureLogitsWarper(temperature)] + ([TopKLogitsWarper(top_k)] if top_k > 0 else []) + \
        ([TopPLogitsWarper(top_p)] if top_p < 1.0 else []) + ([MinPLogitsWarper(min_p)] if min_p else [])
    for p in warpers:
        x = p(None, x)
    return torch.softmax(WO.warp(x[0], kw), -1), x[0]


DRAWS = [  # (temperature, top_k, top_p, min_p, warpers)
    (1.0, 0, 1.0, 0.0, dict(typical_p=0.3)),
    (0.8, 50, 0.95, 0.0, dict(typical_p=0.6)),
    (1.0, 0, 1.0, 0.0, dict(epsilon_cutoff=3e-3)),
    (0.7, 200, 0.9, 0.0, dict(eta_cutoff=0.02)),
    (0.9, 15, 0.85, 0.05, dict(typical_p=0.7, epsilon_cutoff=0.02, eta_cutoff=0.05)),
    (1.2, 0, 0.95, 0.02, dict(epsilon_cutoff=1e-3, eta_cutoff=3e-3)),
]


@pytest.mark.parametrize("temperature,top_k,top_p,min_p,kw", DRAWS)
def test_warper_draws_follow_hf(temperature, top_k, top_p, min_p, kw):
    from genvc_amd.engine import GptEngine, logits_processors, logits_sets, sample_params
    gen = torch.Generator().manual_seed(17)
    s = torch.randn(V, generator=gen) * 2.0
    p_hf, pre = _hf_probs(s, temperature, top_k, top_p, min_p, kw)
    kept = p_hf > 0
    assert 2 <= int(kept.sum()) < int(torch.isfinite(pre).sum())          # the warpers drop ids and leave a choice
    B, n0, steps = 64, 8, 80
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    params = sample_params(dict(repetition_penalty=1.0, temperature=temperature, top_p=top_p, top_k=top_k), V, EOS, seed=11)
    sets = logits_sets([dict(kw, min_p=min_p or None)] * B, n0, V)
    assert (sets.sets is not None) == bool(min_p)
    logits = s.to(DEV).expand(B, V).contiguous()
    counts = torch.zeros(V, dtype=torch.long)
    for step in range(steps):
        ids = torch.ones(B, n0 + 2, device=DEV, dtype=torch.int32)
        ids[:, n0 - 1] = 1024
        ids_len = torch.full((B,), n0, device=DEV, dtype=torch.int32)
        fin = torch.zeros(B, device=DEV, dtype=torch.int32)
        tok = eng.sample_warp(logits, ids, ids_len, fin, params, sets, step)
        counts += torch.bincount(tok.long().cpu(), minlength=V)
    n = B * steps
    assert int(counts[~kept].sum()) == 0, "a draw outside HF's kept set"
    if "typical_p" in kw and len(kw) == 1 and top_k == 0:
        assert not bool(kept[int(torch.argmax(pre))]), "this typical case should exclude the argmax"
    exp = p_hf.double() * n
    obs = counts.double()
    big = exp >= 5
    stat = float(((obs[big] - exp[big]) ** 2 / exp[big]).sum())
    rest_e, rest_o = float(exp[~big & kept].sum()), float(obs[~big & kept].sum())
    dof = int(big.sum()) - 1
    if rest_e > 0:
        stat += (rest_o - rest_e) ** 2 / rest_e
        dof += 1
    z = 3.719          # Wilson-Hilferty: the chi-square quantile at 1 - 1e-4
    crit = dof * (1 - 2 / (9 * dof) + z * math.sqrt(2 / (9 * dof))) ** 3
    assert stat < crit, (stat, crit, dof)
    # the same draws when every row gets its own (identical) entry, and the same on rerun: the sums are deterministic
    ids = torch.ones(B, n0 + 2, device=DEV, dtype=torch.int32)
    a = eng.sample_warp(logits, ids.clone(), torch.full((B,), n0, device=DEV, dtype=torch.int32),
                        torch.zeros(B, device=DEV, dtype=torch.int32), params, sets, 3)
    b = eng.sample_warp(logits, ids.clone(), torch.full((B,), n0, device=DEV, dtype=torch.int32),
                        torch.zeros(B, device=DEV, dtype=torch.int32), params, sets, 3)
    assert torch.equal(a, b)
    del logits_processors
    eng.close()


def test_sample_warp_rejects_bad_values():
    from genvc_amd import _lib
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import GptEngine, WarperSets, sample_params
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    B, n0 = 2, 8
    params = sample_params(dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=0), V, EOS)
    logits = torch.randn(B, V, device=DEV)
    for bad in (_lib.LogitsWarpers(1.0, 0, 0, 0), _lib.LogitsWarpers(0, -0.1, 0, 0), _lib.LogitsWarpers(0, 0, float("nan"), 0),
                _lib.LogitsWarpers(0.5, 0, 0, 1)):
        with pytest.raises(GenvcHipError, match="warpers"):
            eng.sample_warp(logits, torch.ones(B, n0, device=DEV, dtype=torch.int32), torch.full((B,), 4, device=DEV, dtype=torch.int32),
                            torch.zeros(B, device=DEV, dtype=torch.int32), params, WarperSets.one(None, bad, B), 0)
    with pytest.raises(GenvcHipError, match="warpers"):
        ws = WarperSets([None], [_lib.LogitsWarpers(0.5, 0, 0, 0)], [1, 0])
        eng.sample_warp(logits, torch.ones(B, n0, device=DEV, dtype=torch.int32), torch.full((B,), 4, device=DEV, dtype=torch.int32),
                        torch.zeros(B, device=DEV, dtype=torch.int32), params, ws, 0)
    eng.close()


# ---- 5. invariants: off values and a null pointer are bit-identical; greedy, top_k = 1 and beams ignore the warpers -------------
@pytest.mark.parametrize("top_k", [1, 15, 0])
def test_off_entries_and_null_pointer_change_no_kernel_result(top_k):
    from genvc_amd import _lib
    from genvc_amd.engine import GptEngine, WarperSets, sample_params
    gen = torch.Generator().manual_seed(5 + top_k)
    B, n0 = 5, 9
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    params = sample_params(dict(repetition_penalty=2.0, temperature=0.85, top_p=0.85, top_k=top_k), V, EOS, seed=2)
    off = WarperSets.one(None, _lib.LogitsWarpers(), B)
    null = WarperSets.one(None, _lib.LogitsWarpers(), B)
    null.warps = None
    on = WarperSets.one(None, _lib.LogitsWarpers(0.3, 0.01, 0.0, 0), B)
    for step in range(20):
        logits = (torch.randn(B, V, generator=gen) * 3).to(DEV)
        ids = torch.randint(0, V, (B, n0 + 4), generator=gen).int().to(DEV)
        outs = []
        for ws in (None, off, null, on):
            args = (logits, ids.clone(), torch.full((B,), n0, device=DEV, dtype=torch.int32), torch.zeros(B, device=DEV, dtype=torch.int32),
                    params)
            outs.append(eng.sample(*args, step) if ws is None else eng.sample_warp(*args, ws, step))
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), step
        if top_k == 1:
            assert torch.equal(outs[0], outs[3]), step               # the argmax kernel never reads the warpers
    eng.close()


def test_off_values_greedy_and_beams_are_bit_identical(gold):
    g, cond, codes, kw, samp = load_case(gold, "typical")
    s = dict(samp, seed=5)
    for extra in (OFF, dict(typical_p=1.5, epsilon_cutoff=2.0, eta_cutoff=-1.0), dict(typical_p=None)):
        a = g.generate(cond, codes, **s)
        la = g.last_latents.clone()
        b = g.generate(cond, codes, **s, **extra)
        assert torch.equal(a, b) and torch.equal(la, g.last_latents), extra
    # do_sample=False, top_k = 1 and beams: the warpers are not built / never read
    for base in (dict(samp, do_sample=False), dict(samp, top_k=1)):
        a = g.generate(cond, codes, **base)
        la = g.last_latents.clone()
        b = g.generate(cond, codes, **base, **kw, epsilon_cutoff=0.3)
        assert torch.equal(a, b) and torch.equal(la, g.last_latents), base
    fake = g.compute_embeddings(cond, codes)
    pa = list(g.get_generator(fake_inputs=fake, **s))
    pb = list(g.get_generator(fake_inputs=fake, **s, **OFF))
    assert len(pa) == len(pb) and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(pa, pb))
    groups = [(cond[:1], codes[:1]), (cond[1:], codes[1:])]
    oa = g.generate_groups(groups, joint_sampling=True, class_seeds=[1, 2], **samp)
    ob = g.generate_groups(groups, joint_sampling=True, class_seeds=[1, 2], group_kwargs=[OFF, None], **samp)
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    oa = g.generate_rolling(groups, job_seeds=[1, 2], max_rows=2, **samp)
    ob = g.generate_rolling(groups, job_seeds=[1, 2], job_kwargs=[None, OFF], max_rows=2, **samp)
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    beam = dict(num_beams=2, do_sample=False, repetition_penalty=2.0, beam_length_mode="generated")
    a = g.generate(cond, codes, **beam)
    sa = g.last_beam_scores.clone()
    b = g.generate(cond, codes, **beam, **kw)
    assert torch.equal(a, b) and torch.equal(sa, g.last_beam_scores)
    TP._close(g)


# ---- 6. warm path: warper calls neither allocate nor capture ----------------------------------------------------------------------
def test_warper_calls_after_warmup_neither_allocate_nor_capture(gold):
    g, cond, codes, kw, samp = load_case(gold, "harness")
    eng = g.engine
    B = cond.shape[0]
    n0 = 32 + codes.shape[1] + 3
    mx = n0 + g.max_gen_mel_tokens
    for k in (1, 0):
        eng.warmup(B, mx, k)
        eng.warmup_range(B, n0 + 1, mx, k)
    g.generate(cond, codes, **samp)
    base = eng.lazy_inits()
    g.generate(cond, codes, **samp, **kw)
    g.generate(cond, codes, **samp, typical_p=0.3, min_new_tokens=3)
    groups = [(cond[:1], codes[:1]), (cond[1:], codes[1:])]
    g.generate_groups(groups, group_kwargs=[kw, dict(eta_cutoff=0.01)], joint_sampling=True, class_seeds=[1, 2], **samp)
    torch.cuda.synchronize()
    assert eng.lazy_inits() == base
    TP._close(g)
