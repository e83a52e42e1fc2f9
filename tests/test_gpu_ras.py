"""GPU: repetition-aware sampling (include/genvc_hip.h: gvc_logits_ras, gvc_sample_ras, gvc_gpt_generate_ras) against
its CPU restatement tests/ras_oracle.py: the sampler entry point at every edge of the window, GPT.generate replayed step by step from the
device's own logits, the same tokens on every path, the law of the redraw, off is off, and the warm path.

Every exact comparison is screened on the CPU by the oracle alone: a draw counts when u lies at least RO.MARGIN = 1e-5 in probability
from both edges of the bucket it chose.  fp32 expf moves a cumulative mass by about 1e-7 relative, so the screen is a margin of roughly
50 x."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ras_oracle as RO                       # noqa: E402
import test_gpu_processors as TP              # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026
P = 6                  # prompt length of the hand-built rows
STRIDE = 96            # width of their ids buffer


@pytest.fixture(scope="module")
def eng():
    from genvc_amd.engine import GptEngine
    e = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def logits3():
    """the fixed synthetic logits [3, V] of the sampler cases"""
    return synth.uniform(4100, "ras_logits", (3, V), 3.0)


# ---- 1. the sampler entry point against the oracle, exact ------------------------------------------------------------------------
def _filler(rng, n, x):
    """n ids in [0, 1024) none of which is x"""
    f = rng.integers(0, 1024, size=n)
    f[f == x] = (x + 1) % 1024
    return [int(t) for t in f]


# edge -> (window K, min_count, builder(x, rng) -> (row ids, finished, full), redraw expected when x is not the stop token)
def _row(x, rng, prompt_has_x, n_gen, at=(), finished=False, full=False):
    """a row of P prompt ids and n_gen generated ids with x at the generated positions `at` counted from the END (1 = the last id)"""
    prompt = _filler(rng, P, x)
    if prompt_has_x:
        prompt[2] = x
    gen = _filler(rng, n_gen, x)
    for a in at:
        gen[n_gen - a] = x
    return prompt + gen, finished, full


EDGES = {
    "n_gen_0":            (10, 1, lambda x, r: _row(x, r, True, 0), False),
    "short_prompt_only":  (10, 1, lambda x, r: _row(x, r, True, 3), False),
    "short_hit":          (10, 1, lambda x, r: _row(x, r, True, 3, at=(2,)), True),
    "at_len_minus_K":     (10, 1, lambda x, r: _row(x, r, False, 15, at=(10,)), True),
    "at_len_minus_K_1":   (10, 1, lambda x, r: _row(x, r, False, 15, at=(11,)), False),
    "two_of_three":       (10, 3, lambda x, r: _row(x, r, False, 15, at=(1, 7)), False),
    "three_of_three":     (10, 3, lambda x, r: _row(x, r, False, 15, at=(1, 7, 10)), True),
    "K1_hit":             (1, 1, lambda x, r: _row(x, r, False, 5, at=(1,)), True),
    "K1_miss":            (1, 1, lambda x, r: _row(x, r, False, 5, at=(2,)), False),
    "K64_hit":            (64, 1, lambda x, r: _row(x, r, False, 70, at=(64,)), True),
    "K64_miss":           (64, 1, lambda x, r: _row(x, r, False, 70, at=(65,)), False),
    "finished_row":       (10, 1, lambda x, r: _row(x, r, False, 15, at=(1,), finished=True), False),
    "full_buffer":        (10, 1, lambda x, r: _row(x, r, False, STRIDE - P, at=(1,), full=True), False),
}

SETTINGS = {
    "top_k_1":     (dict(repetition_penalty=1.0, temperature=0.85, top_p=1.0, top_k=1), {}),
    "k15_p085":    (dict(repetition_penalty=1.0, temperature=0.85, top_p=0.85, top_k=15), {}),
    "k0_min_p":    (dict(repetition_penalty=1.3, temperature=0.9, top_p=1.0, top_k=0), dict(min_p=0.05)),
    "suppress":    (dict(repetition_penalty=1.3, temperature=1.1, top_p=0.95, top_k=0),
                    dict(suppress_tokens=list(range(0, 1024, 3)), min_new_tokens=80)),      # a third of the ids and the EOS: -inf
}


def _build_case(edge, setting, logits, seed, index=(0, 0, 0), keyed=False):
    """the three rows of a case under `seed`, or None when the oracle's screen refuses the seed: every row's first draw must be the
    token its history was built around (the repetition penalty moves the row when the token enters it) and every draw must clear
    RO.MARGIN.  -> (rows, finished, full, per-row oracle results, keys)"""
    K, mc, build, _ = EDGES[edge]
    samp, kw = SETTINGS[setting]
    step = 7
    rows, fins, fulls, res, keys = [], [], [], [], []
    for b in range(3):
        key = (seed * 31 + 1000 * b + 17, 40 + b + step, 5 - b) if keyed else (seed, step, b)
        ras = (K, mc) if index[b] >= 0 else None
        x = None
        for _ in range(6):                         # fixed point: build around x, draw, rebuild around what was drawn
            rng = np.random.default_rng(1000 * seed + b)
            row, fin, full = build(0 if x is None else x, rng)
            r = RO.step(logits[b], row, P, samp, kw, ras, key, EOS, finished=fin, full=full)
            if r["x"] == x:
                break
            x = r["x"]
        else:
            return None
        if min(r["margin1"], r["margin2"]) < RO.MARGIN:
            return None
        rows.append(row); fins.append(fin); fulls.append(full); res.append(r); keys.append(key)
    return rows, fins, fulls, res, keys


def _pick_seed(edge, setting, logits, **kw):
    for seed in range(1, 4000):
        c = _build_case(edge, setting, logits, seed, **kw)
        if c is not None:
            return seed, c
    raise AssertionError(f"no seed in 1..3999 passes the oracle's screen for {edge} / {setting}")


def _run_case(eng, edge, setting, logits, index=(0, 0, 0), keyed=False):
    from genvc_amd.engine import RasTable, WarperSets, logits_ras, logits_sets, row_sampling, sample_params
    K, mc, _, expect = EDGES[edge]
    samp, kw = SETTINGS[setting]
    seed, (rows, fins, fulls, res, keys) = _pick_seed(edge, setting, logits, index=index, keyed=keyed)
    for r in res:                                   # the screen, re-asserted
        assert min(r["margin1"], r["margin2"]) >= RO.MARGIN
    ids = torch.zeros(3, STRIDE, dtype=torch.int32)
    for b, row in enumerate(rows):
        ids[b, :len(row)] = torch.tensor(row, dtype=torch.int32)
    ids = ids.to(DEV)
    ids_len = torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)
    fin = torch.tensor([int(f) for f in fins], dtype=torch.int32, device=DEV)
    params = sample_params(samp, V, EOS, seed=seed)
    sets = logits_sets([kw] * 3, P, V) if kw else None
    if tuple(index) != (0, 0, 0):
        assert sets is None
        sets = WarperSets([None], [None], list(index))
    ras = logits_ras(dict(ras_window=K), P)
    ras.min_count = mc                              # (hand-set: the cases name their count)
    counters = torch.zeros(3, dtype=torch.int32, device=DEV)
    rws = None
    if keyed:
        rws = row_sampling([dict(samp, seed=k[0], rng_row=k[2], rng_step0=k[1] - 7) for k in keys])
    tok = eng.sample_ras(logits.to(DEV), ids, ids_len, fin, params, RasTable([ras], counters), 7, sets=sets, rows=rws).cpu().tolist()
    cnt = counters.cpu().tolist()
    for b, r in enumerate(res):
        assert tok[b] == r["tok"], (edge, setting, b, tok[b], r)
        assert cnt[b] == int(r["redraw"]), (edge, setting, b, cnt[b], r)
        want = expect and index[b] >= 0 and r["x"] != EOS
        assert r["redraw"] == want, (edge, setting, b, r)
        if not fulls[b]:
            assert int(ids[b, len(rows[b])]) == r["tok"] and int(ids_len[b]) == len(rows[b]) + 1
    return res


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_sampler_entry_matches_oracle_at_every_window_edge(eng, logits3, setting):
    n_redraw = 0
    for edge in EDGES:
        res = _run_case(eng, edge, setting, logits3)
        n_redraw += sum(r["redraw"] for r in res)
        if setting == "suppress":
            for r in res:                           # the redraw respects -inf: no suppressed id, no banned EOS
                assert not r["redraw"] or (r["tok"] != EOS and (r["tok"] >= 1024 or r["tok"] % 3 != 0)), r
    assert n_redraw >= 12


def test_redraw_never_lands_on_an_impossible_id(eng, logits3):
    """the suppress setting at many keys: every redraw's token is neither suppressed nor the banned stop token"""
    from genvc_amd.engine import RasTable, logits_ras, logits_sets, sample_params
    samp, kw = SETTINGS["suppress"]
    samp = dict(samp, repetition_penalty=1.0)          # (the first draw then does not move when its token enters the row)
    sets = logits_sets([kw] * 3, P, V)
    ras = RasTable([logits_ras(dict(ras_window=1, ras_threshold=1.0), P)], torch.zeros(3, dtype=torch.int32, device=DEV))
    lg = logits3.to(DEV)
    seen = 0
    for seed in range(40):
        params = sample_params(samp, V, EOS, seed=seed)
        ids = torch.full((3, STRIDE), 1, dtype=torch.int32, device=DEV)
        n = torch.full((3,), P + 2, dtype=torch.int32, device=DEV)
        fin = torch.zeros(3, dtype=torch.int32, device=DEV)
        first = eng.sample_bias(lg, ids.clone(), n.clone(), fin.clone(), params, None, 3, sets=sets)
        ids[:, P + 1] = first                         # the token the step will draw again is the row's last id: it redraws
        before = ras.redraws.clone()
        tok = eng.sample_ras(lg, ids, n, fin, params, ras, 3, sets=sets)
        assert torch.equal(ras.redraws - before, torch.ones_like(before))
        assert bool(((tok != EOS) & ((tok % 3 != 0) | (tok >= 1024))).all()), tok
        seen += 3
    assert seen == 120


def test_only_the_indexed_row_and_keyed_rows(eng, logits3):
    """row 1 alone carries RAS (indices -1, 0, -1), and keyed rows draw both uniforms from their own keys"""
    for setting in ("top_k_1", "k15_p085"):
        res = _run_case(eng, "short_hit", setting, logits3, index=(-1, 0, -1))
        assert [r["redraw"] for r in res] == [False, True, False]
    for edge in ("at_len_minus_K", "at_len_minus_K_1", "three_of_three"):
        _run_case(eng, edge, "k15_p085", logits3, keyed=True)
        _run_case(eng, edge, "k0_min_p", logits3, keyed=True)


def test_sample_ras_rejects_bad_values(eng, logits3):
    from genvc_amd import _lib
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import RasTable, sample_params
    params = sample_params(SETTINGS["k15_p085"][0], V, EOS)
    for bad in (_lib.LogitsRas(65, 1, P, 0), _lib.LogitsRas(-1, 1, P, 0), _lib.LogitsRas(10, 0, P, 0), _lib.LogitsRas(10, 1, -1, 0),
                _lib.LogitsRas(10, 1, P, 1)):
        with pytest.raises(GenvcHipError, match="ras") as e:
            eng.sample_ras(logits3.to(DEV), torch.ones(3, STRIDE, device=DEV, dtype=torch.int32),
                           torch.full((3,), P, device=DEV, dtype=torch.int32), torch.zeros(3, device=DEV, dtype=torch.int32), params,
                           RasTable([bad]), 0)
        assert e.value.code == -1          # GVC_ERR_ARG


# ---- 2. GPT.generate end to end: every step replayed by the oracle from the device's own logits and history ------------------------
MAX_NEW = 48
E2E = {
    # B, generate kwargs, RAS kwargs, replay from ("logits": the raw row through the oracle's chain; "scores": the stored row itself)
    "b2_k15_p085_K10": (2, dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=1.2), dict(ras_window=10), "logits"),
    "top_k_1_K4":      (1, dict(top_k=1, temperature=0.85, repetition_penalty=1.0), dict(ras_window=4), "logits"),
    # guidance_scale with num_return_sequences > 1 is refused by the guided path as before this feature (NotImplementedError), so the
    # two halves of that configuration run one by one.  The guided row is not the raw conditional row: with nothing truncated
    # (top_k = 0, top_p = 1) the stored scores row IS the row both draws are taken from, and the replay reads it.  Over 1026 nearly
    # even ids nothing repeats by chance: a repetition penalty below 1 rewards the ids of the row, which is the loop RAS is there to break
    "guidance_1p5":    (2, dict(top_k=0, top_p=1.0, temperature=0.7, repetition_penalty=0.5, guidance_scale=1.5), dict(ras_window=10),
                        "scores"),
    "nrs2_k15":        (1, dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=1.2, num_return_sequences=2), dict(ras_window=10),
                        "logits"),
}


def _inputs(B, seed=31, Tc=7):
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    cond = synth.uniform(seed, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(seed, "content_codes", (B, Tc), 256).to(DEV)
    return cond, codes


@pytest.mark.parametrize("one_launch", ["1", "0"], ids=["one_launch_steps", "launch_per_phase"])
@pytest.mark.parametrize("case", list(E2E))
def test_generate_replays_step_by_step(case, one_launch, monkeypatch):
    from genvc_amd.engine import ras_counts
    monkeypatch.setenv("GVC_PERSIST", one_launch)
    monkeypatch.setenv("GVC_PERSIST_ROWS", one_launch)
    B, gkw, rkw, source = E2E[case]
    g, _ = TP.make_gpt(gcfg.TINY_MODEL_ARGS, 3)
    cond, codes = _inputs(B)
    extra = {}
    if "guidance_scale" in gkw:
        extra = dict(negative_cond_latents=synth.uniform(77, "neg", (1, 32, cond.shape[2]), 1.0).to(DEV))
    seed = 5
    out = g.generate(cond, codes, seed=seed, max_new_tokens=MAX_NEW, group=8, return_dict_in_generate=True, output_logits=True,
                     output_scores=True, **gkw, **rkw, **extra)
    toks = out.sequences.cpu()
    rows_n, n = toks.shape
    N = gkw.get("num_return_sequences", 1)
    assert rows_n == B * N and n <= MAX_NEW
    fake = g.compute_embeddings(cond, codes).cpu()
    plen = int(fake.shape[1])
    samp = dict(repetition_penalty=gkw["repetition_penalty"], temperature=gkw["temperature"], top_p=gkw.get("top_p", 1.0), top_k=gkw["top_k"])
    ras = ras_counts(rkw)
    redraws = out.ras_redraws.cpu().tolist()
    assert torch.equal(out.ras_redraws, g.last_ras_redraws)
    n_re = n_plain = n_excused = n_steps = 0
    for r in range(rows_n):
        row = [int(t) for t in fake[r // N]]
        fin, row_re, row_exc = False, 0, 0
        for t in range(n):
            if source == "logits":
                o = RO.step(out.logits[t][r].cpu(), row, plen, samp, {}, ras, (seed, t, r), EOS, finished=fin)
            else:
                # the stored row: what the first draw was taken from, and -- nothing being truncated -- the row of the redraw
                s = out.scores[t][r].cpu()
                x, m1 = RO.draw(s, O_rng(seed, t, r))
                c = RO.count(row, plen, ras[0], x)
                o = dict(x=x, tok=x, redraw=False, margin1=m1, margin2=float("inf"), c=c)
                if c >= ras[1] and x != EOS and not fin:
                    o["tok"], o["margin2"] = RO.draw(s, O_rng(seed ^ RO.SALT, t, r))
                    o["redraw"] = True
                if fin:
                    o["tok"] = EOS
            got = int(toks[r, t])
            if not fin:
                n_steps += 1
                if min(o["margin1"], o["margin2"]) < RO.MARGIN:
                    n_excused += 1
                    row_exc += 1
                else:
                    assert got == o["tok"], (case, r, t, got, o)
                    n_re += int(o["redraw"])
                    n_plain += int(not o["redraw"])
                # the device's flag, as far as the tokens show it: a token other than the first draw can only come from a redraw
                row_re += int(o["redraw"]) if got == o["tok"] else int(got != o["x"])
            else:
                assert got == EOS
            row.append(got)
            fin = fin or got == EOS
        assert abs(redraws[r] - row_re) <= row_exc, (case, r, redraws[r], row_re, row_exc)
    print(f"{case} [{one_launch}]: {n_steps} live steps, {n_re} redraws and {n_plain} plain steps compared, {n_excused} excused, "
          f"device counters {redraws}")
    assert n_excused <= 0.05 * n_steps
    assert n_re >= 3 and n_plain >= 3
    # scores and logits are those of the first draw: the call without RAS stores the same rows as long as the tokens agree
    base = g.generate(cond, codes, seed=seed, max_new_tokens=MAX_NEW, group=8, return_dict_in_generate=True, output_logits=True,
                      output_scores=True, **gkw, **extra)
    same = 0
    while same < min(n, base.sequences.shape[1]) and torch.equal(base.sequences[:, same], out.sequences[:, same]):
        same += 1
    for t in range(min(same + 1, n, base.sequences.shape[1])):
        assert torch.equal(base.scores[t], out.scores[t]) and torch.equal(base.logits[t], out.logits[t]), (case, t)
    assert "ras_redraws" not in base and g.last_ras_redraws is None
    TP._close(g)


def O_rng(seed, step, row):
    from oracle.genvc_oracle import rng_uniform
    return rng_uniform(seed, step, row)


# ---- 3. the same tokens on every path ----------------------------------------------------------------------------------------------
# (a repetition penalty below 1 rewards the ids of the row: repeats, and with them redraws, are common in 32 steps)
SAMP3 = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=0.7, do_sample=True, max_new_tokens=32)
RAS3 = dict(ras_window=10, ras_threshold=0.2)


def test_generator_groups_and_rolling_give_the_tokens_of_generate():
    g, _ = TP.make_gpt(gcfg.TINY_MODEL_ARGS, 3)
    cond, codes = _inputs(3)
    want = g.generate(cond[:2], codes[:2], seed=5, **SAMP3, **RAS3)
    n_re = int(g.last_ras_redraws.sum())
    assert n_re >= 3
    assert not torch.equal(want, g.generate(cond[:2], codes[:2], seed=5, **SAMP3))          # RAS changes the tokens of this call
    fake = g.compute_embeddings(cond[:2], codes[:2])
    pairs = list(g.get_generator(fake_inputs=fake, stream_group=8, seed=5, **SAMP3, **RAS3))
    assert torch.equal(torch.stack([p[0] for p in pairs], 1), want)
    assert int(g.last_ras_redraws.sum()) == n_re
    # per-item dicts: each item the tokens it gets alone, RAS on one, another window on the next, none on the last
    items = [(cond[:1], codes[:1]), (cond[1:2], codes[1:2]), (cond[2:], codes[2:])]
    kws = [RAS3, dict(ras_window=4), None]
    seeds = [3, 4, 6]
    solo = [g.generate(c, x, seed=s, **SAMP3, **(k or {})) for (c, x), s, k in zip(items, seeds, kws)]
    g.groups_stats = {"joint": 0, "separate": 0}
    outs = g.generate_groups(items, group_kwargs=kws, joint_sampling=True, class_seeds=seeds, group=8, **SAMP3)
    assert g.groups_stats["joint"] == 1
    for o, s in zip(outs, solo):
        assert torch.equal(o, s)
    rolled = g.generate_rolling(items, job_seeds=seeds, job_kwargs=kws, group=8, max_rows=2, **SAMP3)
    for o, s in zip(rolled, solo):
        assert torch.equal(o, s)
    # call-wide RAS, and "greedy with an escape" (top_k = 1 draws: it takes the jobs' seeds)
    outs = g.generate_groups(items[:2], joint_sampling=True, class_seeds=seeds[:2], group=8, **SAMP3, **RAS3)
    for o, (c, x), s in zip(outs, items, seeds):
        assert torch.equal(o, g.generate(c, x, seed=s, **SAMP3, **RAS3))
    g1 = dict(SAMP3, top_k=1, repetition_penalty=1.0)
    rolled = g.generate_rolling(items[:2], job_seeds=seeds[:2], group=8, **g1, ras_window=4)
    for o, (c, x), s in zip(rolled, items, seeds):
        assert torch.equal(o, g.generate(c, x, seed=s, **g1, ras_window=4))
    assert not torch.equal(rolled[0], g.generate(items[0][0], items[0][1], **g1))
    with pytest.raises(NotImplementedError, match="job_seeds"):          # RAS draws: a rolling call needs the jobs' seeds
        g.generate_rolling(items[:2], **g1, ras_window=4)
    del g.groups_stats
    TP._close(g)


def test_stream_session_with_ras_beside_one_without():
    """a session with RAS and one without share every decode call; each gets the tokens and waveform of its solo run"""
    from genvc_amd.inference.inference_utils import segments, synthesize_utt_streaming
    from genvc_amd.inference.model_init import model_init_synthetic
    from genvc_amd.streaming import StreamSessions
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=8)[0]
    m.gpt.max_gen_mel_tokens = 30
    cfg = m.config
    saved = dict(top_k=cfg.top_k, top_p=cfg.top_p, temperature=cfg.temperature, repetition_penalty=cfg.repetition_penalty)
    refs = [synth.synth_audio(60 + i, "ref", 72000) for i in range(2)]
    srcs = [synth.synth_audio(80 + i, "src", n) for i, n in enumerate((32000, 16000))]
    segs = [list(segments(s, 16000, 5120)) for s in srcs]
    setting = dict(top_k=1, top_p=1.0, temperature=0.8, repetition_penalty=1.0)
    seeds = [3, 4]
    ras = [dict(ras_window=4), None]

    def solo(i, gk):
        for k, v in dict(saved, **setting).items():
            setattr(cfg, k, v)
        try:
            r = synthesize_utt_streaming(m, srcs[i], refs[i], seg_len=1.0, stream_chunk_size=8, verbose=False, return_details=True,
                                         generate_kwargs=dict(gk or {}, seed=seeds[i]))
        finally:
            for k, v in saved.items():
                setattr(cfg, k, v)
        return torch.cat(r["tokens"], 1)[0].cpu(), r["wav"].cpu(), r.get("ras_redraws")

    ss = StreamSessions(m, max_sessions=2, group=8, per_session_sampling=True)
    sids, wavs = {}, {}
    for i in range(2):
        sids[i] = ss.open(refs[i], sampling=setting, seed=seeds[i], generate_kwargs=ras[i])
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
    for i in range(2):
        toks, wav, counts = solo(i, ras[i])
        got = torch.cat(ss.close(sids[i]), 1)[0].cpu()
        assert torch.equal(got, toks), f"session {i}: tokens differ from its solo run"
        np.testing.assert_allclose(torch.cat(wavs[sids[i]], -1).cpu().numpy(), wav.numpy(), atol=2e-4)
        if ras[i] is not None:
            assert len(counts) == len(segs[i]) and sum(counts) >= 1          # the details carry the redraws of every segment
            assert not torch.equal(toks, solo(i, None)[0]), "RAS changes nothing in this session"
        else:
            assert counts is None
    del m
    torch.cuda.empty_cache()


# ---- 4. the law of the redraw ------------------------------------------------------------------------------------------------------
def test_redraw_follows_the_mixture_of_truncated_and_full():
    """fixed logits and a history whose last generated id is `a`, the likeliest token of the truncated set, under K = 1: a draw of a, and
    only of a, is thrown away.  Law: P_trunc(x) [x != a] + P_trunc(a) P_full(x).  20 480 draws, chi-square with the pooling of
    test_sampler_draws_follow_softmax_of_the_processed_scores (expected count >= 5, the rest pooled), p-value > 1e-4; no draw on a
    suppressed id"""
    from scipy import stats
    from genvc_amd.engine import GptEngine, RasTable, logits_ras, logits_sets, sample_params
    R, calls = 64, 320
    samp = dict(repetition_penalty=1.0, temperature=0.85, top_p=0.85, top_k=15)
    kw = dict(suppress_tokens=list(range(100, 200)))
    lg = synth.uniform(4200, "ras_law", (1, V), 3.0)[0]
    probe = RO.truncated_row(RO.full_row(lg, [1] * P, P, samp, kw, EOS), samp, kw)
    a = int(torch.argmax(probe))
    row = [1] * P + [2, a]
    full = RO.full_row(lg, row, P, samp, kw, EOS)
    p_full = torch.softmax(full.double(), -1).numpy()
    p_trunc = torch.softmax(RO.truncated_row(full, samp, kw).double(), -1).numpy()
    law = p_trunc.copy()
    law[a] = 0.0
    law += p_trunc[a] * p_full
    assert abs(law.sum() - 1.0) < 1e-9 and 0.05 < p_trunc[a] < 0.6
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    logits = lg[None].expand(R, V).contiguous().to(DEV)
    ids = torch.zeros(R, 64, dtype=torch.int32, device=DEV)
    ids[:, :len(row)] = torch.tensor(row, dtype=torch.int32, device=DEV)
    fin = torch.zeros(R, dtype=torch.int32, device=DEV)
    sp = sample_params(samp, V, EOS, seed=4242)
    sets = logits_sets([kw] * R, P, V)
    ras = RasTable([logits_ras(dict(ras_window=1, ras_threshold=1.0), P)], torch.zeros(R, dtype=torch.int32, device=DEV))
    counts = np.zeros(V, dtype=np.int64)
    for step in range(calls):
        ids_len = torch.full((R,), len(row), dtype=torch.int32, device=DEV)
        tok = eng.sample_ras(logits, ids, ids_len, fin, sp, ras, step, sets=sets)
        counts += np.bincount(tok.cpu().numpy(), minlength=V)
    n = R * calls
    n_re = int(ras.redraws.sum())
    assert counts.sum() == n
    assert counts[100:200].sum() == 0 and counts[law == 0].sum() == 0, "a draw on an impossible id"
    # the redraws themselves: Binomial(n, P_trunc(a)) within five standard deviations
    assert abs(n_re - n * p_trunc[a]) < 5 * np.sqrt(n * p_trunc[a] * (1 - p_trunc[a]))
    exp = law * n
    big = exp >= 5
    obs_b = np.append(counts[big], counts[~big].sum())
    exp_b = np.append(exp[big], exp[~big].sum())
    keep = exp_b > 0
    chi2 = float(((obs_b[keep] - exp_b[keep]) ** 2 / exp_b[keep]).sum())
    dof = int(keep.sum()) - 1
    pv = float(stats.chi2.sf(chi2, dof))
    print(f"redraw law: a = {a}, P_trunc(a) = {p_trunc[a]:.4f}, {n_re} redraws of {n} draws, chi2 {chi2:.1f} / dof {dof}, p-value {pv:.3g}")
    assert pv > 1e-4
    eng.close()


# ---- 5. off is off -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [1, 15, 0])
def test_off_entries_null_table_and_no_index_change_no_kernel_result(eng, top_k):
    from genvc_amd.engine import RasTable, WarperSets, logits_ras, sample_params
    gen = torch.Generator().manual_seed(50 + top_k)
    B, n0 = 3, 9
    params = sample_params(dict(repetition_penalty=2.0, temperature=0.85, top_p=0.85, top_k=top_k), V, EOS, seed=2)
    on = logits_ras(dict(ras_window=10), n0 - 4)
    for step in range(20):
        logits = (torch.randn(B, V, generator=gen) * 3).to(DEV)
        ids = torch.randint(0, 40, (B, n0 + 4), generator=gen).int().to(DEV)

        def args():
            return (logits, ids.clone(), torch.full((B,), n0, device=DEV, dtype=torch.int32), torch.zeros(B, device=DEV, dtype=torch.int32),
                    params)
        base = eng.sample(*args(), step)
        cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
        w0 = eng.sample_ras(*args(), RasTable([None], cnt), step)                                               # window == 0
        none = eng.sample_ras(*args(), RasTable([on], cnt), step, sets=WarperSets([None], [None], [-1] * B))     # every index -1
        null = eng._sample("sample_ras", *args(), step, None, [None, None, 1, None, None, None, None])          # a null table
        assert torch.equal(base, w0) and torch.equal(base, none) and torch.equal(base, null), step
        assert int(cnt.sum()) == 0


@pytest.mark.parametrize("top_k", [1, 15, 0])
def test_off_spellings_change_nothing_in_generate(top_k):
    """ras_window=None and 0 are the call without the kwarg: tokens, scores, logits and latents bit for bit, the same decode-step
    launches and no lazy initialisation beyond the first call's"""
    g, _ = TP.make_gpt(gcfg.TINY_MODEL_ARGS, 3)
    cond, codes = _inputs(2)
    kw = dict(top_k=top_k, top_p=0.85, temperature=0.85, repetition_penalty=1.2, seed=5, max_new_tokens=24, return_dict_in_generate=True,
              output_scores=True, output_logits=True)
    eng = g.engine

    def run(**extra):
        before = (eng.rows_step_launches(), eng.one_stream_steps())
        out = g.generate(cond, codes, **kw, **extra)
        torch.cuda.synchronize()
        return out, g.last_latents.clone(), (eng.rows_step_launches() - before[0], eng.one_stream_steps() - before[1])
    a, la, na = run()
    lazy = eng.lazy_inits()
    for extra in (dict(ras_window=None), dict(ras_window=0), dict(ras_window=None, ras_threshold=None)):
        b, lb, nb = run(**extra)
        assert torch.equal(a.sequences, b.sequences) and torch.equal(la, lb) and na == nb, extra
        assert all(torch.equal(x, y) for x, y in zip(a.scores, b.scores)) and all(torch.equal(x, y) for x, y in zip(a.logits, b.logits))
        assert "ras_redraws" not in b and g.last_ras_redraws is None
    assert eng.lazy_inits() == lazy
    TP._close(g)


# ---- 6. the warm path --------------------------------------------------------------------------------------------------------------
def test_ras_calls_after_warmup_neither_allocate_nor_capture():
    from genvc_amd.inference.model_init import model_init_synthetic
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=8)[0]
    g = m.gpt
    g.max_gen_mel_tokens = 24
    eng = g.engine
    m.warmup(seg_len=1.0, streams=1, ref_seconds=3.0, stream_chunk_size=8, top_k=1, ras_window=4)
    wav = torch.zeros(1, 16000, device=DEV)
    wav[:, ::7] = 0.01
    feat = m.content_extractor.extract_content_features(wav)
    codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
    ref = torch.zeros(1, 3 * m.config.audio.sample_rate, device=DEV)
    ref[:, ::5] = 0.01
    cond = m.get_gpt_cond_latents(ref, m.config.audio.sample_rate)
    samp = dict(top_k=1, temperature=0.8, repetition_penalty=1.0, group=8)
    g.generate(cond, codes, **samp)
    torch.cuda.synchronize()
    base = eng.lazy_inits()
    g.generate(cond, codes, **samp, ras_window=4)
    g.generate(cond, codes, **samp, ras_window=4, ras_threshold=0.5, min_new_tokens=3)
    list(g.get_generator(fake_inputs=g.compute_embeddings(cond, codes), stream_group=8, **{k: v for k, v in samp.items() if k != "group"},
                         ras_window=4))
    torch.cuda.synchronize()
    assert eng.lazy_inits() == base
    del m
    torch.cuda.empty_cache()
