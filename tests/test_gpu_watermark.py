"""GPU: the green-list watermark (include/genvc_hip.h: gvc_logits_watermark, gvc_sample_wm, gvc_gpt_generate_wm, gvc_wm_score;
DESIGN.md 4.31) against its CPU restatement tests/watermark_oracle.py (pinned to the installed transformers by
tests/test_watermark_host.py): the sampler entry point at every edge of the table, GPT.generate replayed step by step from the
device's own logits, get_generator, off is off, the warm path, the detector's counts, and the loop closed -- mark, detect, and fail to
detect with another key.

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
import watermark_oracle as WM                 # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
P = 6                  # prompt length of the hand-built rows
STRIDE = 32            # width of their ids buffer
KEY_A, KEY_B = WM.DEFAULT_KEY, 2 ** 62 + 12345


@pytest.fixture(scope="module")
def eng():
    from genvc_amd.engine import GptEngine
    e = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    yield e
    e.close()


_tables = {}


def _entry(wm, vocab):
    """a (gvc_logits_watermark, None) entry whose table is a device tensor of this module (the sampler entry needs no context)"""
    from genvc_amd import _lib
    from genvc_amd.engine import WATERMARK_SCHEMES, WatermarkSettings, watermark_table
    if wm is None:
        return None
    ck = (wm["key"], wm["ratio"], wm["scheme"], vocab)
    if ck not in _tables:
        host = watermark_table(WatermarkSettings(wm["ratio"], 0.0, wm["key"], wm["scheme"], 1), vocab)
        _tables[ck] = host.view(torch.int32).to(DEV)
    t = _tables[ck]
    return _lib.LogitsWatermark(t.data_ptr(), float(wm["bias"]), WATERMARK_SCHEMES[wm["scheme"]], (vocab + 31) // 32, 0), None


def _wm(scheme="lefthash", bias=2.0, key=KEY_A, ratio=0.25):
    return dict(key=key, ratio=ratio, scheme=scheme, bias=bias)


# ---- 1. the sampler entry point against the oracle, exact --------------------------------------------------------------------------
def _prev_with_green(vocab, wm, target):
    """the smallest previous id after which `target` is green"""
    for prev in range(vocab):
        if target in WM.lefthash_lists(vocab, wm["key"], wm["ratio"])[prev]:
            return prev
    raise AssertionError(f"{target} is green after no id")


def _case_rows(vocab, edge, wm):
    """-> per batch row: (ids row, finished, full, logits row [vocab]).  The logits are small noise with two planted ids: `red` at
    10.0 and `green` at 9.0 -- without the mark the argmax is `red`, with a bias of 2.0 it is `green` -- chosen per edge"""
    eos = vocab - 1
    rows = []
    for b in range(3):
        rng = np.random.default_rng(1000 * b + 7)
        lg = synth.uniform(4400 + b, f"wm_logits_{vocab}", (vocab,), 1.5)
        prompt = [int(t) for t in rng.integers(0, vocab - 2, size=P)]
        gen = [int(t) for t in rng.integers(0, vocab - 2, size=5)]
        fin = full = False
        target = None
        if edge in ("prev_0", "prev_31", "prev_32", "prev_Vm3", "prev_Vm2", "prev_Vm1"):
            gen[-1] = {"prev_0": 0, "prev_31": 31, "prev_32": 32, "prev_Vm3": vocab - 3, "prev_Vm2": vocab - 2, "prev_Vm1": vocab - 1}[edge]
        elif edge.startswith("green_"):
            target = {"green_31": 31, "green_32": 32, "green_Vm1": vocab - 1}[edge]
            gen[-1] = _prev_with_green(vocab, wm, target)
        elif edge == "n_gen_0":
            gen = []
        elif edge == "prev_minus_1":
            gen[-1] = -1
        elif edge == "prev_past_V":
            gen[-1] = vocab + 5
        elif edge == "finished_row":
            fin = True
        elif edge == "full_buffer":
            gen = gen + [int(t) for t in rng.integers(0, vocab - 2, size=STRIDE - P - 5)]
            full = True
        row = prompt + gen
        prev = row[-1]
        greens = WM.green_mask(vocab, dict(wm, scheme="lefthash"), prev) if wm["scheme"] == "lefthash" else WM.green_mask(vocab, wm, prev)
        if greens is None:
            greens = torch.zeros(vocab, dtype=torch.bool)
        g_ids = [i for i in range(vocab - 1) if greens[i]]
        r_ids = [i for i in range(vocab - 1) if not greens[i]]
        if target is None:
            target = g_ids[b % len(g_ids)] if g_ids else r_ids[1]
        red = r_ids[(3 * b) % len(r_ids)]
        if edge == "negative_bias":          # the argmax is green and falls behind the runner-up
            lg[target], lg[red] = 10.0, 9.0
        else:
            lg[red], lg[target] = 10.0, 9.0
        rows.append((row, fin, full, lg))          # (green_Vm1 plants the stop code itself: a green stop code is biased like any other)
    return rows


# edge -> (bias, moving: at top_k = 1 the oracle's token with the mark differs from its token without)
EDGES = {
    "prev_0": (2.0, True), "prev_31": (2.0, True), "prev_32": (2.0, True), "prev_Vm3": (2.0, True), "prev_Vm2": (2.0, True),
    "prev_Vm1": (2.0, True), "green_31": (2.0, True), "green_32": (2.0, True), "green_Vm1": (2.0, True), "n_gen_0": (2.0, True),
    "prev_minus_1": (2.0, False), "prev_past_V": (2.0, False), "finished_row": (2.0, False), "full_buffer": (2.0, False),
    "negative_bias": (-2.0, True), "bias_0": (0.0, False),
}
SETTINGS = {
    "greedy":      dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=1),
    "k15_t085":    dict(repetition_penalty=1.0, temperature=0.85, top_p=1.0, top_k=15),
    "k40_p09":     dict(repetition_penalty=1.2, temperature=0.85, top_p=0.9, top_k=40),
    "k0":          dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=0),
    "k0_t07_p098": dict(repetition_penalty=1.3, temperature=0.7, top_p=0.98, top_k=0),
}
STEP = 7


def _oracle(vocab, rows, samp, wms, seed, keys=None, pens=None, kw=None):
    """per-row oracle results under `seed`, or None when the screen refuses it (a draw within RO.MARGIN of a bucket edge, or a
    selfhash row with a tie across rank 40)"""
    res = []
    for b, (row, fin, full, lg) in enumerate(rows):
        key = keys[b] if keys else (seed, STEP, b)
        wm = wms[b]
        r = WM.step(lg, row, P, samp, kw or {}, wm, key, vocab - 1, pen=pens[b] if pens else None, finished=fin, full=full)
        if r["margin1"] < RO.MARGIN:
            return None
        if wm is not None and wm["scheme"] == "selfhash" and samp["top_k"] != 1 and WM.rank_tie(
                RO.truncated_row(PN.full_row(lg, row, P, samp, kw or {}, vocab - 1, pens[b] if pens else None), samp, kw or {})):
            return None
        res.append(r)
    return res


def _pick_seed(*a, **k):
    for seed in range(1, 400):
        res = _oracle(*a[:4], seed, *a[4:], **k)
        if res is not None:
            return seed, res
    raise AssertionError("no seed in 1..399 passes the oracle's screen")


def _device_rows(rows):
    ids = torch.zeros(len(rows), STRIDE, dtype=torch.int32)
    for b, (row, _, _, _) in enumerate(rows):
        ids[b, :len(row)] = torch.tensor(row, dtype=torch.int32)
    return (ids.to(DEV), torch.tensor([len(r[0]) for r in rows], dtype=torch.int32, device=DEV),
            torch.tensor([int(r[1]) for r in rows], dtype=torch.int32, device=DEV), torch.stack([r[3] for r in rows]).to(DEV))


def _run(eng, vocab, rows, samp, seed, res, table, sets=None, rws=None, pen=None):
    from genvc_amd.engine import sample_params
    ids, ids_len, fin, logits = _device_rows(rows)
    tok = eng.sample_wm(logits, ids, ids_len, fin, sample_params(samp, vocab, vocab - 1, seed=seed), table, STEP, sets=sets, rows=rws,
                        pen=pen).cpu().tolist()
    for b, r in enumerate(res):
        assert tok[b] == r["tok"], (b, tok[b], r["tok"], r["margin1"])
        if not rows[b][2]:
            assert int(ids[b, len(rows[b][0])]) == r["tok"] and int(ids_len[b]) == len(rows[b][0]) + 1
        else:
            assert int(ids_len[b]) == STRIDE
    return tok


@pytest.mark.parametrize("scheme", ["lefthash", "selfhash"])
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("vocab", [1026, 70])
def test_sampler_entry_matches_oracle_at_every_table_edge(eng, vocab, setting, scheme):
    from genvc_amd.engine import WatermarkTable
    samp = SETTINGS[setting]
    moved = 0
    for edge, (bias, moving) in EDGES.items():
        wm = _wm(scheme, bias)
        rows = _case_rows(vocab, edge, wm)
        seed, res = _pick_seed(vocab, rows, samp, [wm] * 3)
        plain = [WM.step(lg, row, P, samp, {}, None, (seed, STEP, b), vocab - 1, finished=fin, full=full)
                 for b, (row, fin, full, lg) in enumerate(rows)]
        if setting == "greedy" and scheme == "lefthash":
            # non-vacuity: where the case is marked as moving, the oracle's token with the mark is not its token without (a kernel
            # that ignores the table cannot pass); elsewhere the mark leaves the argmax where it was
            for b in range(3):
                assert (res[b]["tok"] != plain[b]["tok"]) == moving, (edge, b, res[b]["tok"], plain[b]["tok"])
        moved += sum(r["tok"] != q["tok"] for r, q in zip(res, plain))
        _run(eng, vocab, rows, samp, seed, res, WatermarkTable([_entry(wm, vocab)]))
    if setting == "greedy" and scheme == "lefthash":
        assert moved == 3 * sum(1 for e in EDGES.values() if e[1])
    print(f"V={vocab} {setting} {scheme}: the mark moves {moved} of {3 * len(EDGES)} tokens")
    assert moved >= 3


def test_sets_keys_off_entries_and_penalties(eng):
    from genvc_amd.engine import PenaltyTable, WarperSets, WatermarkTable, logits_penalties, row_sampling
    vocab = 1026
    wa, wb = _wm("lefthash", 2.0, KEY_A), _wm("lefthash", 2.0, KEY_B, 0.5)
    rows = _case_rows(vocab, "prev_31", wa)
    for setting in ("greedy", "k15_t085"):
        samp = SETTINGS[setting]
        # one indexed row: row 1 alone carries the mark
        seed, res = _pick_seed(vocab, rows, samp, [None, wa, None])
        plain = [WM.step(lg, row, P, samp, {}, None, (seed, STEP, b), vocab - 1) for b, (row, _, _, lg) in enumerate(rows)]
        if setting == "greedy":
            assert [r["tok"] != q["tok"] for r, q in zip(res, plain)] == [False, True, False]
        _run(eng, vocab, rows, samp, seed, res, WatermarkTable([_entry(wa, vocab)]), sets=WarperSets([None], [None], [-1, 0, -1]))
        # two sets with two keys (and ratios), and an off entry (a null table) beside them
        wms = [wa, wb, None]
        seed, res = _pick_seed(vocab, rows, samp, wms)
        _run(eng, vocab, rows, samp, seed, res, WatermarkTable([_entry(wa, vocab), _entry(wb, vocab), None]),
             sets=WarperSets([None] * 3, [None] * 3, [0, 1, 2]))
        if setting == "greedy":
            assert res[1]["tok"] != plain[1]["tok"] or res[1]["tok"] != res[0]["tok"]
        # keyed rows draw from their own keys
        keys = [(seed * 31 + 1000 * b + 17, 40 + b + STEP, 5 - b) for b in range(3)]
        for s2 in range(1, 400):
            keys = [(s2 * 31 + 1000 * b + 17, 40 + b + STEP, 5 - b) for b in range(3)]
            res = _oracle(vocab, rows, samp, [wa] * 3, s2, keys=keys)
            if res is not None:
                break
        rws = row_sampling([dict(samp, seed=k[0], rng_row=k[2], rng_step0=k[1] - STEP) for k in keys])
        _run(eng, vocab, rows, samp, s2, res, WatermarkTable([_entry(wa, vocab)]), rws=rws)
        # penalties and the mark together: the penalties ahead of the warpers, the mark behind them
        pen = (0.5, 0.25, 0)
        seed, res = _pick_seed(vocab, rows, samp, [wa] * 3, pens=[pen] * 3)
        q = logits_penalties(dict(presence_penalty=pen[0], frequency_penalty=pen[1]), P)
        _run(eng, vocab, rows, samp, seed, res, WatermarkTable([_entry(wa, vocab)]), pen=PenaltyTable([q]))


def test_sample_wm_rejects_bad_values(eng):
    from genvc_amd import _lib
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import WatermarkTable, sample_params
    vocab = 1026
    params = sample_params(SETTINGS["k15_t085"], vocab, vocab - 1)
    good = _entry(_wm(), vocab)[0]

    def args():
        return (torch.zeros(3, vocab, device=DEV), torch.ones(3, STRIDE, device=DEV, dtype=torch.int32),
                torch.full((3,), P, device=DEV, dtype=torch.int32), torch.zeros(3, device=DEV, dtype=torch.int32), params)
    for bias, scheme, words, reserved in ((float("nan"), 0, 33, 0), (float("inf"), 0, 33, 0), (2.0, 2, 33, 0), (2.0, -1, 33, 0),
                                          (2.0, 0, 32, 0), (2.0, 0, 34, 0), (2.0, 0, 33, 1)):
        bad = _lib.LogitsWatermark(good.table, bias, scheme, words, reserved)
        with pytest.raises(GenvcHipError, match="watermark") as e:
            eng.sample_wm(*args(), WatermarkTable([(bad, None)]), 0)
        assert e.value.code == -1          # GVC_ERR_ARG
    for n_sets in (0, 4):                  # outside [1, B]
        with pytest.raises(GenvcHipError) as e:
            eng._sample("sample_wm", *args(), 0, None, [None, None, n_sets, None, None, None, None, None,
                                                         WatermarkTable([(good, None)] * 4).wm])
        assert e.value.code == -1


@pytest.mark.parametrize("top_k", [1, 15, 0])
def test_off_entries_null_table_and_no_index_change_no_kernel_result(eng, top_k):
    from genvc_amd.engine import WarperSets, WatermarkTable, sample_params
    vocab = 1026
    gen = torch.Generator().manual_seed(70 + top_k)
    B, n0 = 3, 9
    params = sample_params(dict(repetition_penalty=2.0, temperature=0.85, top_p=0.85, top_k=top_k), vocab, vocab - 1, seed=2)
    on = WatermarkTable([_entry(_wm(), vocab)])
    for step in range(12):
        logits = (torch.randn(B, vocab, generator=gen) * 3).to(DEV)
        ids = torch.randint(0, 40, (B, n0 + 4), generator=gen).int().to(DEV)

        def args():
            return (logits, ids.clone(), torch.full((B,), n0, device=DEV, dtype=torch.int32), torch.zeros(B, device=DEV, dtype=torch.int32),
                    params)
        base = eng.sample(*args(), step)
        off = eng.sample_wm(*args(), WatermarkTable([None]), step)                                       # an entry with a null table
        none = eng.sample_wm(*args(), on, step, sets=WarperSets([None], [None], [-1] * B))               # every index -1
        null = eng._sample("sample_wm", *args(), step, None, [None, None, 1, None, None, None, None, None, None])      # no entries at all
        assert torch.equal(base, off) and torch.equal(base, none) and torch.equal(base, null), step


# ---- 2. GPT.generate end to end: every step replayed by the oracle from the device's own logits and history ------------------------
MAX_NEW = 32
EOS, V = 1025, 1026
CFG_A = dict(greenlist_ratio=0.25, bias=2.0, hashing_key=KEY_A, seeding_scheme="lefthash", context_width=1)
E2E = {
    # B, generate kwargs, watermarking_config, tolerance of the stored scores (tests/test_gpu_scores.py's, for the same kind of row)
    "greedy_search":     (2, dict(do_sample=False, repetition_penalty=1.2), dict(CFG_A), TS.TOL * 1.2),
    "greedy_renorm":     (1, dict(do_sample=False, repetition_penalty=1.0, renormalize_logits=True), dict(CFG_A, bias=3.0), TS.TOL),
    # truncated rows (TopK / TopP), lefthash and selfhash, and a sampled call with renormalize_logits: TOL / temperature
    "k15_p085":          (2, dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=1.2), dict(CFG_A), TS.TOL / 0.85),
    "k40_selfhash":      (1, dict(top_k=40, top_p=0.95, temperature=0.9, repetition_penalty=1.0), dict(CFG_A, seeding_scheme="selfhash"),
                          TS.TOL / 0.9),
    "k15_renorm":        (1, dict(top_k=15, top_p=0.9, temperature=0.85, repetition_penalty=1.0, renormalize_logits=True), dict(CFG_A),
                          TS.TOL / 0.85),
    "k40_selfhash_renorm": (1, dict(top_k=40, top_p=1.0, temperature=0.9, repetition_penalty=1.0, renormalize_logits=True),
                            dict(CFG_A, seeding_scheme="selfhash", bias=1.5), TS.TOL / 0.9),
    "nrs2_full_row":     (1, dict(top_k=0, top_p=1.0, temperature=0.8, repetition_penalty=1.0, num_return_sequences=2),
                          dict(CFG_A, hashing_key=KEY_B, greenlist_ratio=0.5), TS.TOL / 0.8),
    "guidance_1p5":      (2, dict(top_k=0, top_p=1.0, temperature=1.0, repetition_penalty=1.0, guidance_scale=1.5), dict(CFG_A),
                          TS.TOL * (2 * 1.5 - 1)),
}


def _inputs(B, seed=31, Tc=7):
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    cond = synth.uniform(seed, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(seed, "content_codes", (B, Tc), 256).to(DEV)
    return cond, codes


def _ora_wm(cfg):
    return dict(key=cfg["hashing_key"], ratio=cfg["greenlist_ratio"], scheme=cfg["seeding_scheme"], bias=cfg["bias"])


@pytest.mark.parametrize("one_launch", ["1", "0"], ids=["one_launch_steps", "launch_per_phase"])
@pytest.mark.parametrize("case", list(E2E))
def test_generate_replays_step_by_step(case, one_launch, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST", one_launch)
    monkeypatch.setenv("GVC_PERSIST_ROWS", one_launch)
    B, gkw, cfg, tol = E2E[case]
    wm = _ora_wm(cfg)
    g, _ = TP.make_gpt(gcfg.TINY_MODEL_ARGS, 3)
    cond, codes = _inputs(B)
    extra = {}
    guided = "guidance_scale" in gkw
    if guided:
        extra = dict(negative_cond_latents=synth.uniform(77, "neg", (1, 32, cond.shape[2]), 1.0).to(DEV))
    seed = 5
    common = dict(seed=seed, max_new_tokens=MAX_NEW, group=8, return_dict_in_generate=True, output_logits=True, output_scores=True)
    out = g.generate(cond, codes, **common, **gkw, **extra, watermarking_config=cfg)
    base = g.generate(cond, codes, **common, **gkw, **extra)
    toks = out.sequences.cpu()
    rows_n, n = toks.shape
    N = gkw.get("num_return_sequences", 1)
    assert rows_n == B * N and n <= MAX_NEW
    assert not torch.equal(out.sequences, base.sequences), "the mark changes nothing in this call"
    fake = g.compute_embeddings(cond, codes).cpu()
    plen = int(fake.shape[1])
    sampling = gkw.get("do_sample", True)
    renorm = bool(gkw.get("renormalize_logits"))
    samp = dict(repetition_penalty=gkw["repetition_penalty"], temperature=gkw.get("temperature", 1.0) if sampling else 1.0,
                top_p=gkw.get("top_p", 1.0), top_k=gkw.get("top_k", 0) if sampling else 1)
    same = 0
    while same < min(n, base.sequences.shape[1]) and torch.equal(base.sequences[:, same], out.sequences[:, same]):
        same += 1
    n_cmp = n_excused = n_steps = n_marked = 0
    got_rows, ref_rows = [], []
    for r in range(rows_n):
        row = [int(t) for t in fake[r // N]]
        fin = False
        for t in range(n):
            got = int(toks[r, t])
            if guided:
                # the stored scores row is the row the draw is taken from (nothing is truncated; it carries the bias); the same step of
                # the call without the mark stores the guided row ahead of it (temperature 1)
                s = out.scores[t][r].cpu()
                x, m1 = RO.draw(s, RO.rng_uniform(seed, t, r))
                o = dict(tok=EOS if fin else x, margin1=m1)
                if t <= same and t < base.sequences.shape[1]:
                    got_rows.append(s)
                    ref_rows.append(WM.mark_row(base.scores[t][r].cpu(), wm, row[-1]))
                    n_marked += 1
            else:
                lg = out.logits[t][r].cpu()
                o = WM.step(lg, row, plen, samp, {}, wm, (seed, t, r), EOS, finished=fin, greedy_search=not sampling)
                if wm["scheme"] == "selfhash" and WM.rank_tie(RO.truncated_row(PN.full_row(lg, row, plen, samp, {}, EOS, None), samp, {})):
                    o["margin1"] = 0.0          # (a tie across rank 40: the device keeps more than transformers would)
                if tol is not None:
                    ref = o["scores"]
                    got_rows.append(out.scores[t][r].cpu())
                    ref_rows.append(torch.log_softmax(ref, -1) if renorm else ref)
                    n_marked += int(not torch.equal(ref, WM.step(lg, row, plen, samp, {}, None, (seed, t, r), EOS,
                                                                 greedy_search=not sampling)["scores"]))
            if not fin:
                n_steps += 1
                if o["margin1"] < RO.MARGIN:
                    n_excused += 1
                else:
                    assert got == o["tok"], (case, r, t, got, o["tok"])
                    n_cmp += 1
            else:
                assert got == EOS
            row.append(got)
            fin = fin or got == EOS
    print(f"{case} [{one_launch}]: {n_steps} live steps, {n_cmp} compared, {n_excused} excused; {len(got_rows)} score rows compared, "
          f"{n_marked} of them carrying the bias; the calls with and without the mark agree for {same} steps")
    assert n_excused <= 0.05 * n_steps and n_cmp >= 8
    if tol is not None:
        assert n_marked >= 1
        TS.compare(torch.stack(got_rows)[None], torch.stack(ref_rows)[None], tol, f"{case}: scores")
    # logits stay raw: the call without the mark stores the same rows as long as the histories agree
    for t in range(min(same + 1, n, base.sequences.shape[1])):
        assert torch.equal(base.logits[t], out.logits[t]), (case, t)
    TP._close(g)


SAMP3 = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=1.2, do_sample=True, max_new_tokens=32)


def test_generator_groups_and_rolling_give_the_tokens_of_generate():
    g, _ = TP.make_gpt(gcfg.TINY_MODEL_ARGS, 3)
    cond, codes = _inputs(3)
    want = g.generate(cond[:2], codes[:2], seed=5, **SAMP3, watermarking_config=CFG_A)
    assert not torch.equal(want, g.generate(cond[:2], codes[:2], seed=5, **SAMP3))
    fake = g.compute_embeddings(cond[:2], codes[:2])
    pairs = list(g.get_generator(fake_inputs=fake, stream_group=8, seed=5, **SAMP3, watermarking_config=CFG_A))
    assert torch.equal(torch.stack([p[0] for p in pairs], 1), want)
    # greedy search through the generator
    gs = dict(do_sample=False, repetition_penalty=1.2, max_new_tokens=24)
    wantg = g.generate(cond[:2], codes[:2], **gs, watermarking_config=CFG_A)
    pairs = list(g.get_generator(fake_inputs=fake, stream_group=8, **gs, watermarking_config=CFG_A))
    assert torch.equal(torch.stack([p[0] for p in pairs], 1), wantg)
    # per-item dicts: two keys (and schemes) in one joint call and an item without a mark -- each item the tokens it gets alone
    items = [(cond[:1], codes[:1]), (cond[1:2], codes[1:2]), (cond[2:], codes[2:])]
    cfg_b = dict(CFG_A, hashing_key=KEY_B, greenlist_ratio=0.5, seeding_scheme="selfhash")
    kws = [dict(watermarking_config=CFG_A), dict(watermarking_config=cfg_b), None]
    seeds = [3, 4, 6]
    solo = [g.generate(c, x, seed=s, **SAMP3, **(k or {})) for (c, x), s, k in zip(items, seeds, kws)]
    bare = [g.generate(c, x, seed=s, **SAMP3) for (c, x), s in zip(items, seeds)]
    assert not torch.equal(solo[0], bare[0]) and not torch.equal(solo[1], bare[1]) and torch.equal(solo[2], bare[2])
    g.groups_stats = {"joint": 0, "separate": 0}
    outs = g.generate_groups(items, group_kwargs=kws, joint_sampling=True, class_seeds=seeds, group=8, **SAMP3)
    assert g.groups_stats["joint"] == 1
    for o, s in zip(outs, solo):
        assert torch.equal(o, s)
    rolled = g.generate_rolling(items, job_seeds=seeds, job_kwargs=kws, group=8, max_rows=2, **SAMP3)
    for o, s in zip(rolled, solo):
        assert torch.equal(o, s)
    # a call-wide mark, and a per-item None that switches it off for one item
    wide = [g.generate(c, x, seed=s, **SAMP3, watermarking_config=CFG_A) for (c, x), s in zip(items[:2], seeds)]
    joint = g.groups_stats["joint"]
    outs = g.generate_groups(items[:2], joint_sampling=True, class_seeds=seeds[:2], group=8, **SAMP3, watermarking_config=CFG_A)
    assert g.groups_stats["joint"] == joint + 1
    for o, s in zip(outs, wide):
        assert torch.equal(o, s)
    rolled = g.generate_rolling(items[:2], job_seeds=seeds[:2], group=8, **SAMP3, watermarking_config=CFG_A)
    for o, s in zip(rolled, wide):
        assert torch.equal(o, s)
    outs = g.generate_groups(items[:2], group_kwargs=[None, dict(watermarking_config=None)], joint_sampling=True, class_seeds=seeds[:2],
                             group=8, **SAMP3, watermarking_config=CFG_A)
    assert torch.equal(outs[0], wide[0]) and torch.equal(outs[1], bare[1])
    # greedy rows on the joint paths refuse instead of returning unmarked codes
    with pytest.raises(NotImplementedError, match="watermarking_config with greedy rows"):
        g.generate_groups(items[:2], group=8, **dict(SAMP3, top_k=1), watermarking_config=CFG_A)
    assert all(v == 0 for v in g.engine._wm["holds"].values())          # every finished call gave its slots back
    del g.groups_stats
    TP._close(g)


def test_stream_sessions_with_two_keys_beside_one_without():
    """three sessions share every decode call: two marked under different keys, one unmarked; each gets the tokens of its solo run,
    each marked one is detected with its own key only, and a session holds its table's slot from open to close"""
    from genvc_amd.engine import WatermarkDetector
    from genvc_amd.inference.inference_utils import segments, synthesize_utt_streaming
    from genvc_amd.inference.model_init import model_init_synthetic
    from genvc_amd.streaming import StreamSessions
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=8)[0]
    m.gpt.max_gen_mel_tokens = 30
    cfg = m.config
    saved = dict(top_k=cfg.top_k, top_p=cfg.top_p, temperature=cfg.temperature, repetition_penalty=cfg.repetition_penalty)
    refs = [synth.synth_audio(60 + i, "ref", 72000) for i in range(3)]
    srcs = [synth.synth_audio(80 + i, "src", n) for i, n in enumerate((32000, 16000, 16000))]
    segs = [list(segments(s, 16000, 5120)) for s in srcs]
    setting = dict(top_k=0, top_p=0.95, temperature=1.0, repetition_penalty=1.0)
    seeds = [3, 4, 5]
    cfg_b = dict(CFG_A, hashing_key=KEY_B)
    marks = [dict(watermarking_config=CFG_A, min_new_tokens=30), dict(watermarking_config=cfg_b, min_new_tokens=30), None]

    def solo(i, gk):
        for k, v in dict(saved, **setting).items():
            setattr(cfg, k, v)
        try:
            r = synthesize_utt_streaming(m, srcs[i], refs[i], seg_len=1.0, stream_chunk_size=8, verbose=False, return_details=True,
                                         generate_kwargs=dict(gk or {}, seed=seeds[i]))
        finally:
            for k, v in saved.items():
                setattr(cfg, k, v)
        return torch.cat(r["tokens"], 1)[0].cpu()

    ss = StreamSessions(m, max_sessions=3, group=8, per_session_sampling=True)
    with pytest.raises(NotImplementedError, match="top_k=1"):
        ss.open(refs[0], sampling=dict(setting, top_k=1), seed=1, generate_kwargs=marks[0])
    sids = {}
    for i in range(3):
        sids[i] = ss.open(refs[i], sampling=setting, seed=seeds[i], generate_kwargs=marks[i])
        for sg in segs[i]:
            ss.push(sids[i], sg)
    holds = m.gpt.engine._wm["holds"]
    assert sorted(holds.values()) == [1, 1]
    steps = 0
    while True:
        ss.step()
        steps += 1
        if ss.idle():
            break
        assert steps < 200
    for i in range(3):
        got = torch.cat(ss.close(sids[i]), 1)[0].cpu()
        assert torch.equal(got, solo(i, marks[i])), f"session {i}: tokens differ from its solo run"
        if marks[i] is not None:
            # the session's codes (30 per segment, the stop code held off): its own key finds the mark, the other session's does not
            z = {k: float(WatermarkDetector(c, V)(got[None], return_dict=True)["z_score"][0]) for k, c in (("own", marks[i]["watermarking_config"]),
                 ("other", marks[1 - i]["watermarking_config"]))}
            print(f"session {i}: z with its own key {z['own']:.3f}, with the other session's key {z['other']:.3f}")
            assert z["own"] > 3.0 and z["other"] <= 3.0
    assert all(v == 0 for v in holds.values())
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("top_k", [1, 15, 0])
def test_off_spelling_changes_nothing_in_generate(top_k):
    """None is the call without the kwarg: tokens, scores, logits and latents bit for bit, the same decode-step launches, no table
    uploaded and no lazy initialisation beyond the first call's"""
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
    b, lb, nb = run(watermarking_config=None)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(la, lb) and na == nb
    assert all(torch.equal(x, y) for x, y in zip(a.scores, b.scores)) and all(torch.equal(x, y) for x, y in zip(a.logits, b.logits))
    assert eng.lazy_inits() == lazy and eng.watermark_uploads() == 0
    if top_k != 1:
        c, _, nc = run(watermarking_config=CFG_A)          # (on: other tokens, through the same step launches per step)
        assert not torch.equal(a.sequences, c.sequences) and eng.watermark_uploads() == 1
    TP._close(g)


def test_marked_calls_after_warmup_neither_allocate_upload_nor_capture():
    from genvc_amd.inference.model_init import model_init_synthetic
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=8)[0]
    g = m.gpt
    g.max_gen_mel_tokens = 24
    eng = g.engine
    m.warmup(seg_len=1.0, streams=1, ref_seconds=3.0, stream_chunk_size=8, top_k=1, watermarking_config=CFG_A)
    assert eng.watermark_uploads() == 1
    wav = torch.zeros(1, 16000, device=DEV)
    wav[:, ::7] = 0.01
    feat = m.content_extractor.extract_content_features(wav)
    codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
    ref = torch.zeros(1, 3 * m.config.audio.sample_rate, device=DEV)
    ref[:, ::5] = 0.01
    cond = m.get_gpt_cond_latents(ref, m.config.audio.sample_rate)
    samp = dict(do_sample=False, repetition_penalty=1.0, group=8)
    g.generate(cond, codes, **samp)
    torch.cuda.synchronize()
    base = eng.lazy_inits()
    arena = eng._wm["buf"].data_ptr()
    g.generate(cond, codes, **samp, watermarking_config=CFG_A)
    g.generate(cond, codes, **samp, watermarking_config=dict(CFG_A, bias=1.0), min_new_tokens=3)          # (the bias is no part of the table)
    list(g.get_generator(fake_inputs=g.compute_embeddings(cond, codes), stream_group=8, do_sample=False, watermarking_config=CFG_A))
    torch.cuda.synchronize()
    assert eng.lazy_inits() == base and eng.watermark_uploads() == 1 and eng._wm["buf"].data_ptr() == arena
    assert all(v == 0 for v in eng._wm["holds"].values())          # every finished call gave its slot back
    del m
    torch.cuda.empty_cache()


def test_nine_live_tables_are_refused_and_an_idle_slot_is_reused(eng):
    from genvc_amd.engine import MAX_WATERMARK_TABLES, WatermarkSettings, WatermarkTable
    held = [WatermarkTable([eng.watermark_entry(WatermarkSettings(0.25, 2.0, 100 + i, "selfhash", 1))], eng)
            for i in range(MAX_WATERMARK_TABLES)]
    with pytest.raises(ValueError, match="watermark tables are in use"):
        eng.watermark_entry(WatermarkSettings(0.25, 2.0, 999, "selfhash", 1))
    held[3].release()
    m, key = eng.watermark_entry(WatermarkSettings(0.25, 2.0, 999, "selfhash", 1))          # takes the slot that was given back
    assert m.table == eng._wm["buf"][3].data_ptr() and eng.watermark_uploads() == MAX_WATERMARK_TABLES + 1
    from genvc_amd.engine import watermark_table
    want = watermark_table(WatermarkSettings(0.25, 2.0, 999, "selfhash", 1), 1026).view(torch.int32).reshape(-1)
    assert torch.equal(eng._wm["buf"][3, :want.numel()].cpu(), want)
    eng.watermark_release(key)
    for h in held:
        h.release()


# ---- 3. the detector ----------------------------------------------------------------------------------------------------------------
def _codes(n, seed, vocab=V, lo=0):
    return torch.randint(lo, vocab, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("scheme", ["lefthash", "selfhash"])
def test_detector_counts_and_flags_match_the_oracle(scheme, ignore):
    from genvc_amd.engine import WatermarkDetector
    cfg = dict(CFG_A, seeding_scheme=scheme)
    wm = _ora_wm(cfg)
    det = WatermarkDetector(cfg, V, ignore_repeated_ngrams=ignore)
    for n in (2, 3, 64, 2048):
        # ragged lens, an id >= V and a negative id inside, and (n >= 64) codes drawn from 12 ids so that n-grams repeat
        rows = [_codes(n, 10 + n), _codes(n, 20 + n, vocab=12), _codes(n, 30 + n)]
        lens = [n, n, max(1, n // 2)]
        if n >= 3:
            rows[0][1] = V + 3
            rows[2][0] = -1
        counts, flags = det.counts(torch.tensor(rows), lens=torch.tensor(lens))
        counts, flags = counts.cpu().tolist(), flags.cpu().tolist()
        for b in range(3):
            scored, green, fl = WM.detector_flags(rows[b], lens[b], V, wm, ignore_repeated=ignore)
            assert counts[b] == [scored, green], (n, b, counts[b], scored, green)
            assert flags[b] == fl, (n, b)
        out = det(torch.tensor(rows), lens=torch.tensor(lens), return_dict=True)
        for b in range(3):
            z, p = WM.statistics(*counts[b], cfg["greenlist_ratio"])
            if counts[b][0]:
                assert abs(float(out["z_score"][b]) - z) <= 1e-12 and abs(float(out["p_value"][b]) - p) <= 1e-12
    # a sequence whose every bigram repeats, and one with none
    rep = [5, 9] * 32
    uniq = list(range(100, 164))
    counts, _ = det.counts(torch.tensor([rep, uniq]))
    counts = counts.cpu().tolist()
    for b, row in enumerate((rep, uniq)):
        scored, green, _ = WM.detector_flags(row, 64, V, wm, ignore_repeated=ignore)
        assert counts[b] == [scored, green]
    if ignore:
        assert counts[0][0] == 2 and counts[1][0] == (63 if scheme == "lefthash" else 64)
    else:
        assert counts[0][0] == (63 if scheme == "lefthash" else 64)


def test_detector_rejects_bad_shapes():
    from genvc_amd.engine import WatermarkDetector
    det = WatermarkDetector(CFG_A, V)
    with pytest.raises(ValueError, match="at most 8192"):
        det(torch.zeros(1, 8193, dtype=torch.long))
    with pytest.raises(ValueError, match="codes must be an integer tensor"):
        det(torch.zeros(1, 8))
    with pytest.raises(ValueError, match="lens"):
        det(torch.zeros(2, 8, dtype=torch.long), lens=torch.tensor([8]))


# ---- 4. the loop closed ---------------------------------------------------------------------------------------------------------------
def test_marked_codes_are_detected_with_the_key_and_only_with_it():
    """one fixed-seed sampled call of 96 new codes (min_new_tokens holds the stop code off): z > 3 with the right key, z <= 3 with
    another key, z <= 3 for the unmarked call of the same seed.  The seed and the keys are fixed so that the oracle's detector, on the
    tokens the oracle's replay confirms, meets all three; the device's counts equal the oracle's, so its z is the oracle's"""
    from genvc_amd.engine import WatermarkDetector
    n_new, seed = 96, 11
    g, _ = TP.make_gpt(gcfg.TINY_MODEL_ARGS, 3)
    cond, codes = _inputs(1)
    kw = dict(top_k=0, top_p=0.95, temperature=1.0, repetition_penalty=1.0, seed=seed, max_new_tokens=n_new, min_new_tokens=n_new,
              group=8, return_dict_in_generate=True, output_logits=True)
    out = g.generate(cond, codes, **kw, watermarking_config=CFG_A)
    plainc = g.generate(cond, codes, **kw)
    toks = out.sequences[0].cpu().tolist()
    assert len(toks) == n_new and EOS not in toks
    # the oracle's replay of the marked call from the device's own logits
    fake = g.compute_embeddings(cond, codes).cpu()
    plen = int(fake.shape[1])
    samp = dict(repetition_penalty=1.0, temperature=1.0, top_p=0.95, top_k=0)
    row = [int(t) for t in fake[0]]
    wm = _ora_wm(CFG_A)
    excused = 0
    for t, got in enumerate(toks):
        o = WM.step(out.logits[t][0].cpu(), row, plen, samp, dict(min_new_tokens=n_new), wm, (seed, t, 0), EOS)
        if o["margin1"] < RO.MARGIN:
            excused += 1
        else:
            assert got == o["tok"], (t, got, o["tok"])
        row.append(got)
    assert excused <= 4
    zs = {}
    for name, cfg, seq in (("right key", CFG_A, toks), ("other key", dict(CFG_A, hashing_key=KEY_B), toks),
                           ("unmarked", CFG_A, plainc.sequences[0].cpu().tolist())):
        dev = WatermarkDetector(cfg, V)(torch.tensor([seq]), return_dict=True)
        scored, green, _ = WM.detector_flags(seq, len(seq), V, _ora_wm(cfg))
        z, _ = WM.statistics(scored, green, cfg["greenlist_ratio"])
        assert (int(dev["num_tokens_scored"][0]), int(dev["num_green_tokens"][0])) == (scored, green) and scored == len(seq) - 1
        assert abs(float(dev["z_score"][0]) - z) <= 1e-12
        zs[name] = z
    print(f"z with the right key {zs['right key']:.3f}, with another key {zs['other key']:.3f}, unmarked {zs['unmarked']:.3f}")
    assert zs["right key"] > 3.0 and zs["other key"] <= 3.0 and zs["unmarked"] <= 3.0
    TP._close(g)


def test_wav_form_scores_the_acoustic_codes_of_the_wav():
    from genvc_amd.inference.model_init import model_init_synthetic
    m = model_init_synthetic(gcfg.default_config(tiny=True, with_acoustic=True), seed=5, device=DEV, max_slots=8)[0]
    sr = int(m.config.audio.sample_rate)
    wav = torch.stack([synth.synth_audio(60 + i, "wm_wav", sr) for i in range(2)]).reshape(2, -1).to(DEV)
    codes = m.acoustic_dvae.get_codebook_indices(m.torch_mel_spectrogram_dvae(wav[:, None]))
    a = m.detect_watermark(wav=wav, sr=sr, watermarking_config=CFG_A)
    b = m.detect_watermark(codes=codes, watermarking_config=CFG_A)
    assert np.array_equal(a["num_tokens_scored"], b["num_tokens_scored"]) and np.array_equal(a["num_green_tokens"], b["num_green_tokens"])
    assert torch.equal(a["flags"], b["flags"]) and int(a["num_tokens_scored"][0]) == codes.shape[1] - 1
    with pytest.raises(ValueError, match="codes=... or wav=..."):
        m.detect_watermark(watermarking_config=CFG_A)
    del m
    torch.cuda.empty_cache()
