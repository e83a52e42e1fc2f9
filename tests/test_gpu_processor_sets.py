"""GPU: per-row logits processor sets (include/genvc_hip.h: gvc_sample_proc_sets / gvc_gpt_generate_proc_sets): the sampler kernels
against the call-wide set and the CPU restatement, the fused loop against gvc_gpt_generate_proc on every decode class, each set acting on
its own rows alone, generate_groups(group_kwargs) / generate_rolling(job_kwargs), StreamSessions with per-session processors, and the
warm path."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proc_oracle as PO                      # noqa: E402
import test_gpu_processors as TP              # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402
from genvc_amd.engine import ProcessorSets, logits_processor_sets, sample_params   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(TP.GOLD))


def _stop_len(t):
    """steps of the reference loop over these rows: up to the step where the last row emits the stop token"""
    hit = t == EOS
    return t.shape[1] if not hit.any(1).all() else int(hit.argmax(1).max()) + 1


# ---- 1. the sampler kernels: a mixed batch of 12 rows, 4 sets and rows without one --------------------------------------------
def test_sample_proc_sets_matches_call_wide_sets_and_oracle():
    from genvc_amd.engine import GptEngine
    gen = torch.Generator().manual_seed(21)
    B, n0, L = 12, 9, 24
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    pattern = [0, 1, None, 2, 3, 0, 1, None, 2, 3, 0, 1]
    top_k = [1, 1, 1, 1, 1, 15, 0, 15, 50, 0, 1, 15]           # greedy and sampling rows, each set with a greedy row
    keys = [dict(repetition_penalty=1.0 if top_k[b] == 1 else 1.4, temperature=1.0 if top_k[b] == 1 else 0.8, top_p=0.9,
                 top_k=top_k[b], seed=7 + b, rng_row=b % 3, rng_step0=4) for b in range(B)]
    lens = [n0 + 6] * B
    for b in (4, 9):
        lens[b] = n0                                           # set 3's begin_suppress acts on rows at their prompt length
    lens[1] = lens[6] = lens[11] = n0 + 2                      # set 1's min_new_tokens bans EOS two tokens in
    logits = torch.randn(B, V, generator=gen) * 3
    for b in (1, 6, 11):
        logits[b, EOS] = float(logits[b].max()) + 2.0          # EOS leads these rows: the ban must move them
    ids = torch.randint(0, V, (B, n0 + 16), generator=gen).int()
    # the argmax of every greedy row before the processors, and rows whose history repeats so the n-gram ban hits it
    top = logits.argmax(1)
    for b in range(B):
        x, y = int(ids[b, 3]), int(ids[b, 4])
        if pattern[b] == 0:
            ids[b, 5] = top[b]
            ids[b, lens[b] - 2], ids[b, lens[b] - 1] = x, y    # the row ends with (x, y) and held (x, y, top) before: top is banned
    sets = [dict(no_repeat_ngram_size=3),
            dict(min_new_tokens=4, suppress_tokens=[int(top[1])]),
            dict(suppress_tokens=sorted({int(top[b]) for b in range(B) if pattern[b] == 2}), min_p=0.2),
            dict(begin_suppress_tokens=sorted({int(top[b]) for b in range(B) if pattern[b] == 3}),
                 exponential_decay_length_penalty=(0, 1.5))]
    kws = [None if k is None else sets[k] for k in pattern]
    ps = logits_processor_sets(kws, n0, V)
    assert ps.n_sets == 4 and list(ps.set_of_row) == [-1 if k is None else k for k in pattern]
    common = sample_params(dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=0), V, EOS)
    lg = logits.to(DEV).contiguous()

    def call(fn, *a):
        i2, il = ids.clone().to(DEV), torch.tensor(lens, device=DEV, dtype=torch.int32)
        fin = torch.zeros(B, device=DEV, dtype=torch.int32)
        return fn(lg, i2, il, fin, *a).cpu()
    for step in (0, 3):
        got = call(eng.sample_proc_sets, common, ps, step, keys)
        none = call(eng.sample_rows, keys, step)
        for k in range(ps.n_sets):
            want = call(eng.sample_proc, common, ps.sets[k], step, keys)
            mine = [b for b in range(B) if ps.set_of_row[b] == k]
            assert torch.equal(got[mine], want[mine]), (step, k)
            assert not torch.equal(got[mine], none[mine]), f"set {k} changed nothing"      # every set fires
        rest = [b for b in range(B) if ps.set_of_row[b] < 0]
        assert torch.equal(got[rest], none[rest]), step
        # greedy rows: the argmax of the restated scores
        for b in range(B):
            if top_k[b] != 1:
                continue
            row = ids[b, :lens[b]].tolist()
            s = PO.rep_penalty(logits[b], row, keys[b]["repetition_penalty"])
            if kws[b] is not None:
                s = PO.process(s, row, n0, kws[b], EOS)
            assert int(got[b]) == int(torch.argmax(s)), (step, b)
    # wrong index / set counts are argument errors
    from genvc_amd._lib import GenvcHipError
    with pytest.raises(GenvcHipError):
        call(eng.sample_proc_sets, common, ProcessorSets([ps.sets[0]], [1] + [0] * (B - 1)), 0, keys)
    with pytest.raises(GenvcHipError):
        call(eng.sample_proc_sets, common, ProcessorSets([ps.sets[0]], [-2] + [0] * (B - 1)), 0, keys)
    eng.close()


# ---- 2./3. the fused loop at full size on every decode class --------------------------------------------------------------------
def _run(eng, prefix, mode, arg=None, n=24, group=8):
    B, P = prefix.shape[0], prefix.shape[1]
    slots = torch.arange(B, device=DEV, dtype=torch.int32)
    eng.prefill(slots, prefix, want_outputs=False)
    ids = torch.ones(B, P + 1 + n + 8, device=DEV, dtype=torch.int32)
    ids[:, P] = eng.dims["start_audio_token"]
    ids_len = torch.full((B,), P + 1, device=DEV, dtype=torch.int32)
    fin = torch.zeros(B, device=DEV, dtype=torch.int32)
    toks = torch.full((B, n), EOS, device=DEV, dtype=torch.int32)
    lats = torch.zeros(B, n, eng.d, device=DEV)
    params = sample_params(dict(repetition_penalty=2.0, temperature=1.0, top_p=1.0, top_k=1), V, EOS)
    for i0 in range(0, n, group):
        mk = P + 1 + i0 + group
        if mode == "none":
            eng.generate(slots, ids, ids_len, fin, params, i0, group, toks, lats, max_keys=mk)
        elif mode == "proc":
            eng.generate(slots, ids, ids_len, fin, params, i0, group, toks, lats, max_keys=mk, proc=arg)
        else:
            eng.generate_proc_sets(slots, ids, ids_len, fin, params, arg, i0, group, toks, lats, max_keys=mk)
    return toks.cpu(), lats.cpu(), ids.cpu()


@pytest.mark.parametrize("one_launch", ["1", "0"], ids=["one_launch_steps", "launch_per_phase"])
def test_generate_proc_sets_matches_call_wide_runs(one_launch, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST", one_launch)
    monkeypatch.setenv("GVC_PERSIST_ROWS", one_launch)
    g, dims = TP.make_gpt(gcfg.DEFAULT_MODEL_ARGS, 17, max_slots=16)
    eng = g.engine
    pattern = [0, 1, None, 2, 3]
    for B in (1, 4, 8, 16):
        cond = synth.uniform(40 + B, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
        codes = synth.integers(40 + B, "content_codes", (B, 11), 256).to(DEV).int()
        prefix = eng.prefix_embeddings(cond, codes)
        P = prefix.shape[1]
        tb, lb, ib = _run(eng, prefix, "none")
        want_variant = (3, 5) if one_launch == "1" else (1, 2, 4)
        assert eng.decode_variant() in want_variant, (B, eng.decode_variant())
        # sets built from the baseline: each bans a token its rows would emit, so every set acts on every one of its rows
        idx = [pattern[b % 5] for b in range(B)]
        of = {k: [b for b in range(B) if idx[b] == k] for k in range(4)}
        sets = {0: dict(suppress_tokens=sorted({int(tb[b, 0]) for b in of[0]})),
                1: dict(begin_suppress_tokens=sorted({int(tb[b, 0]) for b in of[1]}), no_repeat_ngram_size=2),
                2: dict(suppress_tokens=sorted({int(tb[b, 2]) for b in of[2]}), min_new_tokens=3, exponential_decay_length_penalty=(2, 1.05)),
                3: dict(suppress_tokens=sorted({int(tb[b, 1]) for b in of[3]}), min_length=P + 1 + 4)}
        ps = logits_processor_sets([None if k is None else sets[k] for k in idx], P + 1, V, sampling=False)
        tm, lm, im = _run(eng, prefix, "sets", ps)
        assert eng.decode_variant() in want_variant, (B, eng.decode_variant())
        for k in range(ps.n_sets):
            mine = [b for b in range(B) if ps.set_of_row[b] == k]
            tk, lk, _ = _run(eng, prefix, "proc", ps.sets[k])
            assert torch.equal(tm[mine], tk[mine]) and torch.equal(lm[mine], lk[mine]), (B, k)
            for b in mine:
                assert not torch.equal(tm[b], tb[b]), f"B={B}: set {k} does not act on row {b}"
        rest = [b for b in range(B) if ps.set_of_row[b] < 0]
        assert torch.equal(tm[rest], tb[rest]) and torch.equal(lm[rest], lb[rest]), B
        if B != 8:
            continue
        # every set acts on its rows alone: dropping one row's set changes that row's ids and no other row's
        for k in range(ps.n_sets):
            r = [b for b in range(B) if ps.set_of_row[b] == k][0]
            drop = [-1 if b == r else ps.set_of_row[b] for b in range(B)]
            _, _, i2 = _run(eng, prefix, "sets", ProcessorSets(list(ps.sets), drop))
            assert not torch.equal(i2[r], im[r]), (k, r)
            others = [b for b in range(B) if b != r]
            assert torch.equal(i2[others], im[others]), (k, r)
        # all -1: the call without processors; one set for every row: gvc_gpt_generate_proc
        t0, l0, _ = _run(eng, prefix, "sets", ProcessorSets([ps.sets[0]], [-1] * B))
        assert torch.equal(t0, tb) and torch.equal(l0, lb)
        t1, l1, _ = _run(eng, prefix, "sets", ProcessorSets([ps.sets[2]], [0] * B))
        tp, lp, _ = _run(eng, prefix, "proc", ps.sets[2])
        assert torch.equal(t1, tp) and torch.equal(l1, lp)
    TP._close(g)


# ---- 4. generate_groups(group_kwargs) / generate_rolling(job_kwargs) ------------------------------------------------------------
def test_groups_and_rolling_with_per_item_kwargs(gold):
    tag = "min_new"
    g, cond, codes, kw = TP.load_case(gold, tag)
    want, base = gold[f"{tag}_tokens"], gold[f"{tag}_base"]
    gr = TP.greedy(gold, tag)
    groups = [(cond[:1], codes[:1]), (cond[1:], codes[1:])]
    g.groups_stats = {"joint": 0, "separate": 0}
    # joint (greedy) path: the processor group matches the executed reference, the other group the call without processors
    outs = g.generate_groups(groups, group_kwargs=[kw, None], group=8, **gr)
    assert g.groups_stats["joint"] == 1
    assert np.array_equal(outs[0].cpu().numpy()[0], TP.trim(want[0]))
    plain = g.generate_groups(groups, group=8, **gr)
    assert torch.equal(outs[1], plain[1])
    outs = g.generate_groups(groups, group_kwargs=[None, kw], group=8, **gr)
    assert torch.equal(outs[0], plain[0])
    w1 = want[1:, :_stop_len(want[1:])]
    assert np.array_equal(outs[1].cpu().numpy(), w1)
    # a second, different set on the other group equals the call-wide run of that set at the same shape; call-wide kwargs merge under
    other = dict(suppress_tokens=[int(plain[0][0, 0])])
    outs = g.generate_groups(groups, group_kwargs=[other, {}], group=8, **gr, **kw)
    wide_o = g.generate_groups(groups, group=8, **gr, **dict(kw, **other))
    wide_k = g.generate_groups(groups, group=8, **gr, **kw)
    assert torch.equal(outs[0], wide_o[0]) and torch.equal(outs[1], wide_k[1])
    assert not torch.equal(outs[0], wide_k[0])
    # serial (sampling) path: each group is its generate(seed=class seed, **its kwargs)
    samp = dict(do_sample=True, top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0)
    outs = g.generate_groups(groups, group_kwargs=[kw, other], class_seeds=[3, 4], group=8, **samp)
    assert torch.equal(outs[0], g.generate(cond[:1], codes[:1], seed=3, **samp, **kw))
    assert torch.equal(outs[1], g.generate(cond[1:], codes[1:], seed=4, **samp, **other))
    # rolling (greedy), two rows in flight: jobs with and without the set
    B = cond.shape[0]
    jobs = groups + [(cond[B - 1:], codes[B - 1:])]
    outs = g.generate_rolling(jobs, job_kwargs=[kw, None, kw], group=8, max_rows=2, **gr)
    assert np.array_equal(outs[0].cpu().numpy()[0], TP.trim(want[0]))
    assert np.array_equal(outs[1].cpu().numpy(), base[1:, :_stop_len(base[1:])])
    assert np.array_equal(outs[2].cpu().numpy()[0], TP.trim(want[B - 1]))
    del g.groups_stats
    TP._close(g)


def test_rolling_with_job_seeds_and_job_kwargs():
    """sampling with job_seeds: every job equals its solo generate(seed=job seed, **its kwargs), whoever shares its steps"""
    from genvc_amd.inference.model_init import model_init_synthetic
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=16)[0]
    g = m.gpt
    KW = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0, do_sample=True, num_beams=1)
    d = g.model_dim
    mk = [(synth.uniform(90 + i, "cond_latents", (b, 32, d), 1.0).to(DEV), synth.integers(90 + i, "content_codes", (b, tc), 256).to(DEV))
          for i, (b, tc) in enumerate(((5, 40), (6, 25)))]
    jobs = [mk[0], mk[1], mk[1], mk[0], (mk[1][0][:5].contiguous(), mk[1][1][:5].contiguous())]
    jb, seeds = [20, 7, 13, 9, 16], [5, 6, 7, 8, 2 ** 40 + 3]
    jk = [dict(no_repeat_ngram_size=2), None, dict(suppress_tokens=[3, 4, 5], min_new_tokens=5), dict(min_p=0.1), None]
    rolled = g.generate_rolling(jobs, group=5, job_seeds=seeds, job_kwargs=jk, **dict(KW, max_new_tokens=jb))
    for (c, t), a, nb, s, k in zip(jobs, rolled, jb, seeds, jk):
        assert a.shape[1] <= nb and torch.equal(a, g.generate(c, t, **dict(KW, seed=s, max_new_tokens=nb, **(k or {}))))
    del m
    torch.cuda.empty_cache()


# ---- 5. StreamSessions: per-session processors -----------------------------------------------------------------------------------
def test_stream_sessions_per_session_processors():
    """three sessions with processors opened at different times, and one without, each get the tokens and waveform of their solo
    synthesize_utt_streaming(generate_kwargs=...)"""
    from genvc_amd.inference.inference_utils import segments, synthesize_utt_streaming
    from genvc_amd.inference.model_init import model_init_synthetic
    from genvc_amd.streaming import StreamSessions
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=8)[0]
    with torch.inference_mode():
        m.gpt.mel_head.bias[EOS] = 1.8                         # EOS comes early: min_new_tokens has something to ban
    m.gpt.init_gpt_for_inference(max_slots=8)
    m.gpt.max_gen_mel_tokens = 30
    cfg = m.config
    saved = dict(top_k=cfg.top_k, top_p=cfg.top_p, temperature=cfg.temperature, repetition_penalty=cfg.repetition_penalty)
    refs = [synth.synth_audio(60 + i, "ref", 72000) for i in range(4)]
    srcs = [synth.synth_audio(80 + i, "src", n) for i, n in enumerate((32000, 16000, 40000, 24000))]
    segs = [list(segments(s, 16000, 5120)) for s in srcs]
    settings = [dict(top_k=1, repetition_penalty=1.0), dict(top_k=1), dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0),
                dict(top_k=1)]
    seeds = [0, 0, 5, 0]
    procs = [dict(no_repeat_ngram_size=2), dict(min_new_tokens=29), dict(suppress_tokens=[1, 2, 3, 4, 5, 6, 7, 8]), None]

    def solo(i, gk):
        for k, v in dict(saved, **settings[i]).items():
            setattr(cfg, k, v)
        try:
            gk = dict(gk or {}, seed=seeds[i]) if seeds[i] else gk
            r = synthesize_utt_streaming(m, srcs[i], refs[i], seg_len=1.0, stream_chunk_size=8, verbose=False, return_details=True,
                                         generate_kwargs=gk)
        finally:
            for k, v in saved.items():
                setattr(cfg, k, v)
        return torch.cat(r["tokens"], 1)[0].cpu(), r["wav"].cpu()

    ss = StreamSessions(m, max_sessions=4, group=8, per_session_sampling=True)
    sids, wavs = {}, {}
    sids[0] = ss.open(refs[0], sampling=settings[0], seed=seeds[0], generate_kwargs=procs[0])
    ss.push(sids[0], segs[0][0])
    sids[3] = ss.open(refs[3], sampling=settings[3], seed=seeds[3])
    for sg in segs[3]:
        ss.push(sids[3], sg)
    steps = 0
    while True:
        for sid, chunks in ss.step().items():
            wavs.setdefault(sid, []).extend(chunks)
        steps += 1
        if steps == 1:
            sids[1] = ss.open(refs[1], sampling=settings[1], seed=seeds[1], generate_kwargs=procs[1])
            for sg in segs[1]:
                ss.push(sids[1], sg)
            for sg in segs[0][1:]:
                ss.push(sids[0], sg)
        if steps == 3:
            sids[2] = ss.open(refs[2], sampling=settings[2], seed=seeds[2], generate_kwargs=procs[2])
            for sg in segs[2]:
                ss.push(sids[2], sg)
        if steps > 3 and ss.idle():
            break
        assert steps < 200
    got = {i: (torch.cat(ss.close(sids[i]), 1)[0].cpu(), torch.cat(wavs[sids[i]], -1).cpu()) for i in range(4)}
    for i in range(4):
        toks, wav = solo(i, procs[i])
        assert torch.equal(got[i][0], toks), f"session {i}: tokens differ from its solo run"
        assert got[i][1].shape == wav.shape
        np.testing.assert_allclose(got[i][1].numpy(), wav.numpy(), atol=2e-4)
        if procs[i] is not None:
            assert not torch.equal(toks, solo(i, None)[0]), f"session {i}: its processors change nothing"
    with pytest.raises(ValueError):
        ss.open(refs[0], generate_kwargs=dict(top_k=3))
    del m
    torch.cuda.empty_cache()


# ---- 6. warm path -------------------------------------------------------------------------------------------------------------
def test_processor_set_calls_after_warmup_neither_allocate_nor_capture(gold):
    tag = TP.cases(gold, "sampler")[0]
    g, cond, codes, kw = TP.load_case(gold, tag)
    eng = g.engine
    B = cond.shape[0]
    n0 = 32 + codes.shape[1] + 3
    mx = n0 + g.max_gen_mel_tokens
    eng.warmup(B, mx, 1)
    eng.warmup_range(B, n0 + 1, mx, 1)
    g.generate(cond, codes, **TP.GREEDY)
    base = eng.lazy_inits()
    groups = [(cond[:1], codes[:1]), (cond[1:], codes[1:])]
    g.generate_groups(groups, group_kwargs=[kw, dict(no_repeat_ngram_size=3, suppress_tokens=[5])], **TP.GREEDY)
    g.generate_groups(groups, group_kwargs=[None, kw], **TP.GREEDY)
    torch.cuda.synchronize()
    assert eng.lazy_inits() == base
    TP._close(g)
