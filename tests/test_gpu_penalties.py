"""GPU: the presence / frequency / windowed repetition penalties (include/genvc_hip.h: gvc_logits_penalties, gvc_sample_pen,
gvc_gpt_generate_pen) against their CPU restatement tests/penalty_oracle.py: the sampler entry point at every edge of
the history, GPT.generate replayed step by step from the device's own logits, the same tokens on every path, off is off, and the warm
path.

Every exact comparison of a draw is screened on the CPU by the oracle alone, as in tests/test_gpu_ras.py: a draw counts when u lies at
least RO.MARGIN = 1e-5 in probability from both edges of the bucket it chose.  At top_k = 1 nothing is drawn: the scores are the same
fp32 operations on the same inputs on both sides, and the argmax is compared as it is."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import penalty_oracle as PN                   # noqa: E402
import ras_oracle as RO                       # noqa: E402
import test_gpu_processors as TP              # noqa: E402
import test_gpu_scores as TS                  # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026
P = 6                  # prompt length of the hand-built rows
STRIDE = 704           # width of their ids buffer: a history of 620 generated ids fits (counts past 255)
LONG = 620


@pytest.fixture(scope="module")
def eng():
    from genvc_amd.engine import GptEngine
    e = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    yield e
    e.close()


def _logits3():
    """the fixed synthetic logits [3, V] of the sampler cases"""
    return synth.uniform(4300, "penalty_logits", (3, V), 3.0)


@pytest.fixture(scope="module")
def logits3():
    return _logits3()


# ---- 1. the sampler entry point against the oracle, exact ------------------------------------------------------------------------
def _target(lg, which):
    """the id a history is built around: the row's largest logit, its second largest, or the first id 1.0 .. 2.5 below the largest"""
    order = torch.argsort(lg, descending=True)
    if which == "top1":
        return int(order[0])
    if which == "top2":
        return int(order[1])
    for i in order:
        if 1.0 <= float(lg[order[0]] - lg[i]) <= 2.5 and int(i) < 1024:
            return int(i)
    raise AssertionError("no mid-ranked id")


def _filler(rng, n, a):
    """n ids in [0, 1024) none of which is a"""
    f = rng.integers(0, 1024, size=n)
    f[f == a] = (a + 1) % 1024
    return [int(t) for t in f]


def _row(a, rng, prompt_has, n_gen, at=(), count=0, junk=False, finished=False, full=False):
    """P prompt ids and n_gen generated ids; a at the generated positions `at` counted from the END (1 = the last id), or `count`
    copies of it spread over the generated ids; junk: a placeholder -1 and an id past the vocabulary among them"""
    prompt = _filler(rng, P, a)
    if prompt_has:
        prompt[2] = a
    gen = _filler(rng, n_gen, a)
    for k in at:
        gen[n_gen - k] = a
    if count:
        for k in rng.choice(n_gen, size=count, replace=False):
            gen[int(k)] = a
    if junk:
        gen[0], gen[2] = -1, V + 77
    return prompt + gen, finished, full


# edge -> (penalties (presence, frequency, window), target id, builder(a, rng) -> (row ids, finished, full), moving: f * c + p on the
# target exceeds the row's top-1 / top-2 gap, so at top_k = 1 and repetition_penalty 1 the token moves)
EDGES = {
    "n_gen_0":           ((0.5, 0.25, 0), "top1", lambda a, r: _row(a, r, True, 0), False),
    "prompt_only":       ((0.5, 0.25, 0), "top1", lambda a, r: _row(a, r, True, 9), False),
    "prompt_only_W8":    ((0.5, 0.25, 8), "top1", lambda a, r: _row(a, r, True, 9), False),
    "window_alone_W8":   ((0.0, 0.0, 8), "top1", lambda a, r: _row(a, r, False, 12, at=(8,)), False),      # (moves only with rep != 1)
    "at_W":              ((0.5, 0.25, 10), "top1", lambda a, r: _row(a, r, False, 15, at=(10,)), True),
    "at_W_plus_1":       ((0.5, 0.25, 10), "top1", lambda a, r: _row(a, r, False, 15, at=(11,)), False),
    "W1_hit":            ((0.5, 0.25, 1), "top1", lambda a, r: _row(a, r, False, 5, at=(1,)), True),
    "W1_miss":           ((0.5, 0.25, 1), "top1", lambda a, r: _row(a, r, False, 5, at=(2,)), False),
    "W_above_n_gen":     ((0.5, 0.25, 50), "top1", lambda a, r: _row(a, r, True, 5, at=(5,)), True),
    "count_1":           ((0.1, 0.2, 0), "top1", lambda a, r: _row(a, r, False, LONG, count=1), True),
    "count_2":           ((0.1, 0.2, 0), "top1", lambda a, r: _row(a, r, False, LONG, count=2), True),
    "count_300":         ((0.1, 0.2, 0), "top1", lambda a, r: _row(a, r, False, LONG, count=300), True),
    # an 8-bit counter sees 0 of 256 and 44 of 300: the first leaves the largest logit alone, the second lifts a mid-ranked id by 0.44
    # instead of 3.0 -- neither then gives the oracle's token
    "count_256":         ((0.5, 0.25, 0), "top1", lambda a, r: _row(a, r, False, LONG, count=256), True),
    "count_300_reward":  ((0.0, -0.01, 0), "mid", lambda a, r: _row(a, r, False, LONG, count=300), True),
    "negative_f_and_p":  ((-0.2, -0.3, 0), "top2", lambda a, r: _row(a, r, False, 15, at=(3,)), True),
    "junk_ids":          ((0.5, 0.25, 0), "top1", lambda a, r: _row(a, r, False, 15, at=(4,), junk=True), True),
    "finished_row":      ((0.5, 0.25, 0), "top1", lambda a, r: _row(a, r, False, 15, at=(1,), finished=True), False),
    "full_buffer":       ((0.5, 0.25, 0), "top1", lambda a, r: _row(a, r, False, STRIDE - P, at=(1,), full=True), False),
}

SETTINGS = {
    "k1":          (dict(repetition_penalty=1.0, temperature=0.85, top_p=1.0, top_k=1), {}),
    "k1_rep":      (dict(repetition_penalty=1.3, temperature=0.85, top_p=1.0, top_k=1), {}),
    "k15_p085":    (dict(repetition_penalty=1.0, temperature=0.85, top_p=0.85, top_k=15), {}),
    "k0_min_p":    (dict(repetition_penalty=1.3, temperature=0.9, top_p=1.0, top_k=0), dict(min_p=0.05)),
    "suppress":    (dict(repetition_penalty=1.3, temperature=1.1, top_p=0.95, top_k=0),
                    dict(suppress_tokens=list(range(0, 1024, 3)), min_new_tokens=700)),      # a third of the ids and the EOS: -inf
}
STEP = 7


def _build_case(edge, setting, logits, seed, index=(0, 0, 0), keyed=False):
    """the three rows of a case under `seed`, or None when the oracle's screen refuses the seed (a draw within RO.MARGIN of a bucket
    edge) -> (rows, finished, full, per-row oracle results, keys, per-row results without penalties, targets)"""
    pen, which, build, _ = EDGES[edge]
    samp, kw = SETTINGS[setting]
    rows, fins, fulls, res, keys, plain, targets = [], [], [], [], [], [], []
    for b in range(3):
        key = (seed * 31 + 1000 * b + 17, 40 + b + STEP, 5 - b) if keyed else (seed, STEP, b)
        a = _target(logits[b], which)
        row, fin, full = build(a, np.random.default_rng(100 + b))
        r = PN.step(logits[b], row, P, samp, kw, pen if index[b] >= 0 else None, key, EOS, finished=fin, full=full)
        if r["margin1"] < RO.MARGIN:
            return None
        rows.append(row); fins.append(fin); fulls.append(full); res.append(r); keys.append(key); targets.append(a)
        plain.append(PN.step(logits[b], row, P, samp, kw, None, key, EOS, finished=fin, full=full))
    return rows, fins, fulls, res, keys, plain, targets


def _pick_seed(edge, setting, logits, **kw):
    for seed in range(1, 4000):
        c = _build_case(edge, setting, logits, seed, **kw)
        if c is not None:
            return seed, c
    raise AssertionError(f"no seed in 1..3999 passes the oracle's screen for {edge} / {setting}")


def _device_rows(rows, fins):
    ids = torch.zeros(len(rows), STRIDE, dtype=torch.int32)
    for b, row in enumerate(rows):
        ids[b, :len(row)] = torch.tensor(row, dtype=torch.int32)
    return (ids.to(DEV), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV),
            torch.tensor([int(f) for f in fins], dtype=torch.int32, device=DEV))


def _table(pen, plen=P):
    from genvc_amd.engine import PenaltyTable, logits_penalties
    q = logits_penalties(dict(presence_penalty=pen[0], frequency_penalty=pen[1], penalty_window=pen[2]), plen)
    assert q is not None
    return PenaltyTable([q])


def _run_case(eng, edge, setting, logits, index=(0, 0, 0), keyed=False):
    from genvc_amd.engine import WarperSets, logits_sets, row_sampling, sample_params
    pen, _, _, moving = EDGES[edge]
    samp, kw = SETTINGS[setting]
    seed, (rows, fins, fulls, res, keys, plain, targets) = _pick_seed(edge, setting, logits, index=index, keyed=keyed)
    for r in res:                                   # the screen, re-asserted
        assert r["margin1"] >= RO.MARGIN
    if setting == "k1":
        # non-vacuity: where the case is marked as moving, the oracle's token with the penalties is not its token without them (a
        # kernel that ignores the table cannot pass); elsewhere the penalties leave the argmax where it was
        for b in range(3):
            if fins[b] or fulls[b]:
                continue
            assert (res[b]["tok"] != plain[b]["tok"]) == (moving and index[b] >= 0), (edge, b, res[b], plain[b])
    ids, ids_len, fin = _device_rows(rows, fins)
    params = sample_params(samp, V, EOS, seed=seed)
    sets = logits_sets([kw] * 3, P, V) if kw else None
    if tuple(index) != (0, 0, 0):
        assert sets is None
        sets = WarperSets([None], [None], list(index))
    rws = None
    if keyed:
        rws = row_sampling([dict(samp, seed=k[0], rng_row=k[2], rng_step0=k[1] - STEP) for k in keys])
    tok = eng.sample_pen(logits.to(DEV), ids, ids_len, fin, params, _table(pen), STEP, sets=sets, rows=rws).cpu().tolist()
    for b, r in enumerate(res):
        assert tok[b] == r["tok"], (edge, setting, b, tok[b], r, plain[b])
        if not fulls[b]:
            assert int(ids[b, len(rows[b])]) == r["tok"] and int(ids_len[b]) == len(rows[b]) + 1
        else:
            assert int(ids_len[b]) == STRIDE
    return res, plain, targets


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_sampler_entry_matches_oracle_at_every_history_edge(eng, logits3, setting):
    moved = 0
    for edge in EDGES:
        res, plain, targets = _run_case(eng, edge, setting, logits3)
        moved += sum(r["tok"] != q["tok"] for r, q in zip(res, plain))
        if setting == "k1_rep":
            # an id present only in the fake prompt: the repetition penalty acts on it without a window and does not act with one
            if edge == "prompt_only":
                assert all(r["tok"] != a for r, a in zip(res, targets))
            if edge == "prompt_only_W8":
                assert all(r["tok"] == a for r, a in zip(res, targets))
            if edge == "window_alone_W8":          # the windowed repetition penalty alone, on an id inside the window
                assert all(r["tok"] != a for r, a in zip(res, targets))
        if setting == "k1" and edge == "count_300_reward":
            assert all(r["tok"] == a for r, a in zip(res, targets))          # 300 x 0.01 lifts the mid-ranked id to the top; 44 x 0.01 would not
    if setting == "k1":
        assert moved == 3 * sum(1 for e in EDGES.values() if e[3])


def test_only_the_indexed_row_and_keyed_rows(eng, logits3):
    """row 1 alone carries the penalties (indices -1, 0, -1), and keyed rows draw from their own keys"""
    for setting in ("k1", "k15_p085"):
        res, plain, _ = _run_case(eng, "at_W", setting, logits3, index=(-1, 0, -1))
        if setting == "k1":
            assert [r["tok"] != q["tok"] for r, q in zip(res, plain)] == [False, True, False]
    for edge in ("at_W", "at_W_plus_1", "count_300", "negative_f_and_p"):
        _run_case(eng, edge, "k15_p085", logits3, keyed=True)
        _run_case(eng, edge, "k0_min_p", logits3, keyed=True)
    _run_case(eng, "at_W", "k1", logits3, keyed=True)


@pytest.mark.parametrize("setting", ["k1", "k15_p085", "k0_min_p"])
def test_ras_and_penalties_together(eng, logits3, setting):
    """the first draw x comes from the penalised row; x in the RAS window is thrown away and drawn again from the full penalised row.
    The penalties count the last two generated ids (the row's largest logit, twice); x sits third from the end, inside the RAS window of
    four and outside the penalties' window, so the history built around x does not move x"""
    from genvc_amd.engine import RasTable, logits_ras, logits_sets, sample_params
    samp, kw = SETTINGS[setting]
    ras = (4, 1)
    pen = (0.5, 0.25, 2)
    lg = logits3

    def build(seed):
        rows, res = [], []
        for b in range(3):
            a = _target(lg[b], "top1")
            x = None
            for _ in range(8):
                rng = np.random.default_rng(100 + b)
                gen = _filler(rng, 12, a)
                gen[-1] = gen[-2] = a
                if x is not None:
                    gen[-3] = x
                row = _filler(rng, P, a) + gen
                r = PN.step(lg[b], row, P, samp, kw, pen, (seed, STEP, b), EOS, ras=ras)
                if r["x"] == x:
                    break
                x = r["x"]
            else:
                return None
            if min(r["margin1"], r["margin2"]) < RO.MARGIN or not r["redraw"]:
                return None
            rows.append(row); res.append(r)
        return rows, res
    for seed in range(1, 4000):
        c = build(seed)
        if c is not None:
            break
    else:
        raise AssertionError(f"no seed in 1..3999 passes the oracle's screen for {setting}")
    rows, res = c
    assert all(min(r["margin1"], r["margin2"]) >= RO.MARGIN and r["redraw"] for r in res)
    ids, ids_len, fin = _device_rows(rows, [False] * 3)
    counters = torch.zeros(3, dtype=torch.int32, device=DEV)
    rt = logits_ras(dict(ras_window=ras[0]), P)
    rt.min_count = ras[1]
    tok = eng.sample_pen(lg.to(DEV), ids, ids_len, fin, sample_params(samp, V, EOS, seed=seed), _table(pen), STEP,
                         sets=logits_sets([kw] * 3, P, V) if kw else None, ras=RasTable([rt], counters)).cpu().tolist()
    assert tok == [r["tok"] for r in res], (tok, res)
    assert counters.cpu().tolist() == [1, 1, 1]


def test_sample_pen_rejects_bad_values(eng, logits3):
    from genvc_amd import _lib
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import PenaltyTable, sample_params
    params = sample_params(SETTINGS["k15_p085"][0], V, EOS)

    def args():
        return (logits3.to(DEV), torch.ones(3, STRIDE, device=DEV, dtype=torch.int32), torch.full((3,), P, device=DEV, dtype=torch.int32),
                torch.zeros(3, device=DEV, dtype=torch.int32), params)
    for bad in (_lib.LogitsPenalties(2.5, 0.0, 0, P), _lib.LogitsPenalties(0.0, -2.5, 0, P), _lib.LogitsPenalties(float("nan"), 0.0, 0, P),
                _lib.LogitsPenalties(0.0, float("inf"), 0, P), _lib.LogitsPenalties(0.5, 0.0, -1, P), _lib.LogitsPenalties(0.5, 0.0, 0, -1)):
        with pytest.raises(GenvcHipError, match="penalties") as e:
            eng.sample_pen(*args(), PenaltyTable([bad]), 0)
        assert e.value.code == -1          # GVC_ERR_ARG
    good = _lib.LogitsPenalties(0.5, 0.0, 0, P)
    for n_sets in (0, 4):                  # outside [1, B]
        with pytest.raises(GenvcHipError) as e:
            eng._sample("sample_pen", *args(), 0, None, [None, None, n_sets, None, None, None, None, PenaltyTable([good] * 4).pen])
        assert e.value.code == -1


# ---- 2. off is off (the sampler entry) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [1, 15, 0])
def test_off_entries_null_table_and_no_index_change_no_kernel_result(eng, top_k):
    from genvc_amd.engine import PenaltyTable, WarperSets, sample_params
    gen = torch.Generator().manual_seed(70 + top_k)
    B, n0 = 3, 9
    params = sample_params(dict(repetition_penalty=2.0, temperature=0.85, top_p=0.85, top_k=top_k), V, EOS, seed=2)
    on = _table((0.5, 0.5, 0), n0 - 4)
    for step in range(20):
        logits = (torch.randn(B, V, generator=gen) * 3).to(DEV)
        ids = torch.randint(0, 40, (B, n0 + 4), generator=gen).int().to(DEV)

        def args():
            return (logits, ids.clone(), torch.full((B,), n0, device=DEV, dtype=torch.int32), torch.zeros(B, device=DEV, dtype=torch.int32),
                    params)
        base = eng.sample(*args(), step)
        off = eng.sample_pen(*args(), PenaltyTable([None]), step)                                             # an entry with everything off
        none = eng.sample_pen(*args(), on, step, sets=WarperSets([None], [None], [-1] * B))                   # every index -1
        null = eng._sample("sample_pen", *args(), step, None, [None, None, 1, None, None, None, None, None])  # a null table
        assert torch.equal(base, off) and torch.equal(base, none) and torch.equal(base, null), step


# ---- 3. GPT.generate end to end: every step replayed by the oracle from the device's own logits and history ------------------------
MAX_NEW = 32
E2E = {
    # B, generate kwargs, penalty kwargs, tolerance of the stored scores (tests/test_gpu_scores.py's, for the same kind of row)
    "greedy_search_W8":  (2, dict(do_sample=False, repetition_penalty=1.2), dict(presence_penalty=0.4, frequency_penalty=0.2, penalty_window=8),
                          TS.TOL * 1.2),                     # greedy rows: TOL * max(rep, 1)
    "top_k_1_sampled":   (1, dict(top_k=1, temperature=0.85, repetition_penalty=1.0), dict(presence_penalty=0.5, frequency_penalty=0.25),
                          TS.TOL / 0.85),                    # TopK(1) rows: TOL / temperature
    "k15_p085":          (2, dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=1.2),
                          dict(presence_penalty=0.3, frequency_penalty=0.15, penalty_window=8), None),      # (tokens only: a truncated row)
    "nrs2_full_row":     (1, dict(top_k=0, top_p=1.0, temperature=0.8, repetition_penalty=1.0, num_return_sequences=2),
                          dict(presence_penalty=0.4, frequency_penalty=0.2, penalty_window=6), TS.TOL / 0.8),
    "guidance_1p5":      (2, dict(top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, guidance_scale=1.5),
                          dict(presence_penalty=0.6, frequency_penalty=0.3), TS.TOL * (2 * 1.5 - 1)),      # guided rows: TOL * (2 s - 1)
}


def _inputs(B, seed=31, Tc=7):
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    cond = synth.uniform(seed, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(seed, "content_codes", (B, Tc), 256).to(DEV)
    return cond, codes


@pytest.mark.parametrize("one_launch", ["1", "0"], ids=["one_launch_steps", "launch_per_phase"])
@pytest.mark.parametrize("case", list(E2E))
def test_generate_replays_step_by_step(case, one_launch, monkeypatch):
    from genvc_amd.engine import penalty_settings
    monkeypatch.setenv("GVC_PERSIST", one_launch)
    monkeypatch.setenv("GVC_PERSIST_ROWS", one_launch)
    B, gkw, pkw, tol = E2E[case]
    g, _ = TP.make_gpt(gcfg.TINY_MODEL_ARGS, 3)
    cond, codes = _inputs(B)
    extra = {}
    guided = "guidance_scale" in gkw
    if guided:
        extra = dict(negative_cond_latents=synth.uniform(77, "neg", (1, 32, cond.shape[2]), 1.0).to(DEV))
    seed = 5
    common = dict(seed=seed, max_new_tokens=MAX_NEW, group=8, return_dict_in_generate=True, output_logits=True, output_scores=True)
    out = g.generate(cond, codes, **common, **gkw, **pkw, **extra)
    base = g.generate(cond, codes, **common, **gkw, **extra)
    toks = out.sequences.cpu()
    rows_n, n = toks.shape
    N = gkw.get("num_return_sequences", 1)
    assert rows_n == B * N and n <= MAX_NEW
    assert not torch.equal(out.sequences, base.sequences), "the penalties change nothing in this call"
    fake = g.compute_embeddings(cond, codes).cpu()
    plen = int(fake.shape[1])
    sampling = gkw.get("do_sample", True)
    samp = dict(repetition_penalty=gkw["repetition_penalty"], temperature=gkw.get("temperature", 1.0), top_p=gkw.get("top_p", 1.0),
                top_k=gkw.get("top_k", 0) if sampling else 1)
    pen = penalty_settings(pkw)
    # the steps up to and including the first at which the two calls' tokens differ see the same history in both calls
    same = 0
    while same < min(n, base.sequences.shape[1]) and torch.equal(base.sequences[:, same], out.sequences[:, same]):
        same += 1
    n_cmp = n_excused = n_steps = n_pen = 0
    got_rows, ref_rows = [], []
    for r in range(rows_n):
        row = [int(t) for t in fake[r // N]]
        fin = False
        for t in range(n):
            got = int(toks[r, t])
            if guided:
                # the guided row is not the raw conditional row: the stored scores row is the row the draw is taken from (nothing is
                # truncated), and the same step of the call without penalties stores the guided row ahead of them (temperature 1)
                s = out.scores[t][r].cpu()
                x, m1 = RO.draw(s, RO.rng_uniform(seed, t, r))
                o = dict(tok=EOS if fin else x, margin1=m1)
                if t <= same and t < base.sequences.shape[1]:
                    got_rows.append(s)
                    ref_rows.append(PN.penalised(base.scores[t][r].cpu(), row, plen, 1.0, pen))
                    n_pen += int(bool((PN.counts(row, plen, pen[2], V) > 0).any()))
            else:
                lg = out.logits[t][r].cpu()
                o = PN.step(lg, row, plen, samp, {}, pen, (seed, t, r), EOS, finished=fin)
                if tol is not None:
                    got_rows.append(out.scores[t][r].cpu())
                    full = PN.full_row(lg, row, plen, samp, {}, EOS, pen, temperature=sampling)
                    ref_rows.append(RO.truncated_row(full, samp, {}) if sampling and samp["top_k"] == 1 else full)
                    n_pen += int(bool((PN.counts(row, plen, pen[2], V) > 0).any()))
            if not fin:
                n_steps += 1
                if o["margin1"] < RO.MARGIN:
                    n_excused += 1
                else:
                    assert got == o["tok"], (case, r, t, got, o)
                    n_cmp += 1
            else:
                assert got == EOS
            row.append(got)
            fin = fin or got == EOS
    print(f"{case} [{one_launch}]: {n_steps} live steps, {n_cmp} compared, {n_excused} excused; {len(got_rows)} score rows compared, "
          f"{n_pen} of them with a penalised id; the calls with and without penalties agree for {same} steps")
    assert n_excused <= 0.05 * n_steps and n_cmp >= 8
    if tol is not None:
        assert n_pen >= 1
        TS.compare(torch.stack(got_rows)[None], torch.stack(ref_rows)[None], tol, f"{case}: scores")
    # logits stay raw: the call without penalties stores the same rows as long as the histories agree
    for t in range(min(same + 1, n, base.sequences.shape[1])):
        assert torch.equal(base.logits[t], out.logits[t]), (case, t)
    TP._close(g)


# ---- 4. the same tokens on every path ----------------------------------------------------------------------------------------------
SAMP3 = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=1.2, do_sample=True, max_new_tokens=32)
PEN3 = dict(presence_penalty=0.6, frequency_penalty=0.3, penalty_window=12)


def test_generator_groups_and_rolling_give_the_tokens_of_generate():
    g, _ = TP.make_gpt(gcfg.TINY_MODEL_ARGS, 3)
    cond, codes = _inputs(3)
    want = g.generate(cond[:2], codes[:2], seed=5, **SAMP3, **PEN3)
    assert not torch.equal(want, g.generate(cond[:2], codes[:2], seed=5, **SAMP3))          # the penalties change the tokens of this call
    fake = g.compute_embeddings(cond[:2], codes[:2])
    pairs = list(g.get_generator(fake_inputs=fake, stream_group=8, seed=5, **SAMP3, **PEN3))
    assert torch.equal(torch.stack([p[0] for p in pairs], 1), want)
    # per-item dicts: each item the tokens it gets alone -- penalties on one, a windowed repetition penalty on the next, none on the last
    items = [(cond[:1], codes[:1]), (cond[1:2], codes[1:2]), (cond[2:], codes[2:])]
    kws = [PEN3, dict(penalty_window=4), None]
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
    # call-wide penalties, sampled ...
    outs = g.generate_groups(items[:2], joint_sampling=True, class_seeds=seeds[:2], group=8, **SAMP3, **PEN3)
    for o, (c, x), s in zip(outs, items, seeds):
        assert torch.equal(o, g.generate(c, x, seed=s, **SAMP3, **PEN3))
    # ... and greedy (no seeds: the call-wide penalties still count from each item's own prompt): the joint decode of a call-wide
    # setting is the joint decode of the same setting per item, and not that of the call without it
    g1 = dict(SAMP3, top_k=1, repetition_penalty=1.0)
    wide = g.generate_groups(items[:2], group=8, **g1, **PEN3)
    per = g.generate_groups(items[:2], group_kwargs=[PEN3, PEN3], group=8, **g1)
    bare = g.generate_groups(items[:2], group=8, **g1)
    assert all(torch.equal(a, b) for a, b in zip(wide, per)) and not all(torch.equal(a, b) for a, b in zip(wide, bare))
    rolled = g.generate_rolling(items[:2], group=8, **g1, **PEN3)
    per = g.generate_rolling(items[:2], job_kwargs=[PEN3, PEN3], group=8, **g1)
    assert all(torch.equal(a, b) for a, b in zip(rolled, per))
    assert not all(torch.equal(a, b) for a, b in zip(rolled, g.generate_rolling(items[:2], group=8, **g1)))
    del g.groups_stats
    TP._close(g)


def test_stream_session_with_penalties_beside_one_without():
    """a session with penalties and one without share every decode call; each gets the tokens and waveform of its solo run"""
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
    pens = [dict(presence_penalty=0.8, frequency_penalty=0.4, penalty_window=16), None]

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

    ss = StreamSessions(m, max_sessions=2, group=8, per_session_sampling=True)
    sids, wavs = {}, {}
    for i in range(2):
        sids[i] = ss.open(refs[i], sampling=setting, seed=seeds[i], generate_kwargs=pens[i])
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
        toks, wav = solo(i, pens[i])
        got = torch.cat(ss.close(sids[i]), 1)[0].cpu()
        assert torch.equal(got, toks), f"session {i}: tokens differ from its solo run"
        np.testing.assert_allclose(torch.cat(wavs[sids[i]], -1).cpu().numpy(), wav.numpy(), atol=2e-4)
        if pens[i] is not None:
            assert not torch.equal(toks, solo(i, None)[0]), "the penalties change nothing in this session"
    del m
    torch.cuda.empty_cache()


# ---- 5. off is off (generate) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [1, 15, 0])
def test_off_spellings_change_nothing_in_generate(top_k):
    """None and 0 are the call without the kwargs: tokens, scores, logits and latents bit for bit, the same decode-step launches and no
    lazy initialisation beyond the first call's"""
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
    for extra in (dict(presence_penalty=None), dict(presence_penalty=0, frequency_penalty=0.0, penalty_window=0),
                  dict(frequency_penalty=None, penalty_window=None), dict(penalty_window=0)):
        b, lb, nb = run(**extra)
        assert torch.equal(a.sequences, b.sequences) and torch.equal(la, lb) and na == nb, extra
        assert all(torch.equal(x, y) for x, y in zip(a.scores, b.scores)) and all(torch.equal(x, y) for x, y in zip(a.logits, b.logits))
    assert eng.lazy_inits() == lazy
    c, _, _ = run(presence_penalty=0.5, frequency_penalty=0.25, penalty_window=4)          # (on: other tokens)
    assert not torch.equal(a.sequences, c.sequences)
    TP._close(g)


# ---- 6. the warm path --------------------------------------------------------------------------------------------------------------
def test_penalty_calls_after_warmup_neither_allocate_nor_capture():
    from genvc_amd.inference.model_init import model_init_synthetic
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=8)[0]
    g = m.gpt
    g.max_gen_mel_tokens = 24
    eng = g.engine
    pen = dict(presence_penalty=0.5, frequency_penalty=0.25, penalty_window=8)
    m.warmup(seg_len=1.0, streams=1, ref_seconds=3.0, stream_chunk_size=8, top_k=1, **pen)
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
    g.generate(cond, codes, **samp, **pen)
    g.generate(cond, codes, **samp, presence_penalty=1.0, min_new_tokens=3)
    g.generate(cond, codes, **dict(samp, do_sample=False), **pen)
    list(g.get_generator(fake_inputs=g.compute_embeddings(cond, codes), stream_group=8, **{k: v for k, v in samp.items() if k != "group"},
                         **pen))
    torch.cuda.synchronize()
    assert eng.lazy_inits() == base
    del m
    torch.cuda.empty_cache()
