"""CPU: the group (diverse) beam search restatement (tests/group_beam_oracle.py) against the plain restatements and the executed
reference wherever the semantics allow (G = 1; group 0 is a plain search of S beams), a hand-computed step, the fixture
(tests/golden/group_beam.npz, scripts/make_group_beam_golden.py), the kwarg rules and the C ABI."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402
import group_beam_oracle as GO                # noqa: E402
import nbest_oracle as NO                     # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAGS = ["a0", "a1", "a2", "a3", "b0", "b1", "c0", "c1", "d"]
SYMBOLS = ("gvc_group_beam_select", "gvc_gpt_group_beam_generate", "gvc_gpt_warmup_group_beam")
EOS = 1025


def oracle_of(gold, tag):
    margs = gcfg.DEFAULT_MODEL_ARGS if int(gold[f"{tag}_full"]) else gcfg.TINY_MODEL_ARGS
    dims = gcfg.gpt_dims(margs)
    w = synth.make_weights(int(gold[f"{tag}_seed"]), synth.gpt_weight_spec(dims))
    if float(gold[f"{tag}_stop_bias"]) != 0.0:
        w["mel_head.bias"][EOS] = float(gold[f"{tag}_stop_bias"])
    B, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (B, Tc), 256)
    return BO.OracleGpt(w, dims), cond, codes


@pytest.fixture(scope="module")
def tiny():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    w = synth.make_weights(31, synth.gpt_weight_spec(dims))
    w["mel_head.bias"][EOS] = 1.6
    cond = synth.uniform(5003, "cond_latents", (2, 32, dims["d_model"]), 1.0)
    codes = synth.integers(5003, "content_codes", (2, 11), 256)
    return BO.OracleGpt(w, dims), cond, codes


@pytest.mark.parametrize("mode,early,lp", [("4.33", False, 1.0), ("generated", "never", 0.5), ("generated", True, 1.0)])
def test_one_group_is_the_plain_search(tiny, mode, early, lp):
    ora, cond, codes = tiny
    a = GO.group_beam_search(ora, cond, codes, 4, 1, 0.0, lp, 2.0, 24, mode=mode, early_stopping=early, num_return=4)
    b = NO.beam_search(ora, cond, codes, 4, lp, 2.0, 24, mode=mode, early_stopping=early, num_return=4)
    assert a["ids"].shape == b["ids"].shape and np.array_equal(a["ids"], b["ids"])
    assert np.array_equal(a["scores"], b["scores"]) and a["steps"] == b["steps"]
    assert a["min_gap"] == b["min_gap"] and a["order_gap"] == b["order_gap"]


@pytest.mark.parametrize("K,G,lam", [(4, 2, 1.0), (6, 3, 1.0), (4, 4, 0.5)])
def test_group_0_is_a_plain_search_of_S_beams(tiny, K, G, lam):
    """no earlier group penalises group 0: its kept set is the one a plain search with S beams keeps"""
    ora, cond, codes = tiny
    S = K // G
    r = GO.group_beam_search(ora, cond, codes, K, G, lam, 1.0, 2.0, 24, mode="generated", num_return=K)
    p = NO.beam_search(ora, cond, codes, S, 1.0, 2.0, 24, mode="generated", num_return=S) if S > 1 else None
    for b in range(2):
        kept = r["kept"][b][0][::-1]                          # best first
        if S == 1:
            assert len(kept) == 1                             # (the plain restatement needs K >= 2)
            continue
        assert len(kept) == S
        for j, (sc, tk) in enumerate(kept):
            row = p["ids"][b * S + j]
            assert row[:len(tk)].tolist() == tk and bool((row[len(tk):] == EOS).all())
            assert abs(sc - p["scores"][b * S + j]) <= 1e-6


def _executed_cases():
    for name, tags in (("beam_search.npz", ("a", "b", "c")), ("nbest.npz", NO.TAGS)):
        for tag in tags:
            yield name, tag


@pytest.mark.parametrize("name,tag", list(_executed_cases()))
def test_group_0_returns_what_the_executed_reference_returned(name, tag):
    """a group search with G = 2 and 2K beams: group 0's best hypothesis is the sequence the reference's K-beam search returned"""
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gold = dict(np.load(os.path.join(GOLDEN, name)))
    K = int(gold[f"{tag}_K"])
    assert K >= 2
    ora, cond, codes = oracle_of(gold, tag)
    B = int(gold[f"{tag}_B"])
    seen = set()
    for i in range(int(gold[f"{tag}_n"])):
        p = f"{tag}_{i}_"
        lp = float(gold[p + "lp"])
        early = NO.EARLY[int(gold[p + "early"])] if p + "early" in gold else False
        N = int(gold[p + "N"]) if p + "N" in gold else 1
        if (lp, str(early)) in seen:                          # (runs that differ in N alone are one search)
            continue
        seen.add((lp, str(early)))
        r = GO.group_beam_search(ora, cond, codes, 2 * K, 2, 1.0, lp, float(gold[f"{tag}_rep"]), int(gold[f"{tag}_max_new"]),
                                 mode="generated", early_stopping=early, num_return=1)
        for b in range(B):
            tk = r["kept"][b][0][-1][1]
            row = gold[p + "ids"][b * N]
            assert row[:len(tk)].tolist() == tk[:len(row)] and bool((row[len(tk):] == EOS).all()), (tag, i, b)


def _hand_step(group0_done):
    """V = 6 (eos 5), K = 4, G = 2, lambda 1, no repetition penalty, lp 1, mode "generated", t = 2 (so len = 3)"""
    P = torch.tensor([[0.50, 0.20, 0.12, 0.08, 0.06, 0.04],
                      [0.10, 0.60, 0.12, 0.08, 0.06, 0.04],
                      [0.50, 0.30, 0.15, 0.02, 0.02, 0.01],
                      [0.28, 0.25, 0.05, 0.05, 0.05, 0.32]])
    scores = torch.tensor([-1.0, -1.5, -0.5, -0.1])
    ids = torch.full((4, 5), 4, dtype=torch.long)            # (rep = 1: the ids do not matter)
    gen = [[4, 4], [4, 3], [3, 4], [3, 3]]
    hyps = [[BO.Hyps(2), BO.Hyps(2)]]
    done = [[group0_done, False]]
    out = GO.select_step(torch.log(P), ids, scores, gen, hyps, done, 2, 3, 4, 2, 1.0, 6, 5, 1.0, 1.0, "generated")
    return out, hyps, done


def test_hand_computed_step():
    ln = math.log
    (tok, par, sc, gen, _), hyps, done = _hand_step(False)
    # group 0: (row 0, token 0) -1 + ln .5, (row 1, token 1) -1.5 + ln .6; no eos in its top 4
    # group 1: tokens 0 and 1 cost lambda each.  eos of row 3 (-.1 + ln .32) leads and becomes a hypothesis; then (row 2, token 0)
    # ln .5 - .5 - 1, (row 3, token 0) ln .28 - .1 - 1, ahead of (row 2, token 2) ln .15 - .5 and (row 2, token 1) ln .3 - .5 - 1
    assert tok.tolist() == [0, 1, 0, 0] and par.tolist() == [0, 1, 2, 3]
    np.testing.assert_allclose(sc.numpy(), [-1 + ln(.5), -1.5 + ln(.6), ln(.5) - 1.5, ln(.28) - 1.1], rtol=1e-6)
    assert gen == [[4, 4, 0], [4, 3, 1], [3, 4, 0], [3, 3, 0]]
    assert hyps[0][0].items == [] and len(hyps[0][1].items) == 1
    assert hyps[0][1].items[0][1] == [3, 3] and abs(hyps[0][1].items[0][0] - (ln(.32) - .1) / 3) < 1e-6
    assert done == [[False, False]]
    # group 0 done: its rows keep their beams and count as eos twice, so group 1's eos costs 2 lambda and leaves the top 4 (uncounted it
    # would be at rank 1 and become a hypothesis); tokens 0 and 1 are free again
    (tok, par, sc, gen, _), hyps, done = _hand_step(True)
    assert tok.tolist() == [5, 5, 0, 0] and par.tolist() == [0, 1, 2, 3]
    np.testing.assert_allclose(sc.numpy(), [-1.0, -1.5, ln(.5) - .5, ln(.28) - .1], rtol=1e-6)
    assert hyps[0][1].items == [] and done == [[True, False]]
    assert ln(.32) - .1 > ln(.28) - .1 > ln(.32) - .1 - 2.0               # (what the counted eos entries decide)


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_fixture(tag):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gold = dict(np.load(os.path.join(GOLDEN, "group_beam.npz")))
    ora, cond, codes = oracle_of(gold, tag)
    B, K, G, lam = int(gold[f"{tag}_B"]), int(gold[f"{tag}_K"]), int(gold[f"{tag}_G"]), float(gold[f"{tag}_lam"])
    for i in range(int(gold[f"{tag}_n"])):
        p = f"{tag}_{i}_"
        proc = json.loads(str(gold[p + "proc"])) or None
        r = GO.group_beam_search(ora, cond, codes, K, G, lam, float(gold[p + "lp"]), float(gold[f"{tag}_rep"]), int(gold[f"{tag}_max_new"]),
                                 mode=str(gold[p + "mode"]), early_stopping=NO.EARLY[int(gold[p + "early"])], num_return=K, proc_kw=proc)
        assert r["ids"].shape == gold[p + "ids"].shape and np.array_equal(r["ids"], gold[p + "ids"])
        np.testing.assert_allclose(r["scores"], gold[p + "scores"], rtol=1e-5)
        assert r["min_gap"] >= 1e-3 and float(gold[p + "min_gap"]) >= 1e-3
        assert r["order_gap"] >= 1e-3 and float(gold[p + "order_gap"]) >= 1e-3
        sc = r["scores"].reshape(B, K)
        assert bool((sc[:, :-1] > sc[:, 1:]).all())
        # row 0 of every item is the num_return_sequences = 1 result
        w1 = gold[p + "ids1"].shape[1]
        assert np.array_equal(gold[p + "ids1"], r["ids"][::K, :w1]) and bool((r["ids"][::K, w1:] == EOS).all())
        np.testing.assert_allclose(gold[p + "scores1"], r["scores"][::K], rtol=1e-5)


def test_fixture_cases_cover_the_issue():
    gold = dict(np.load(os.path.join(GOLDEN, "group_beam.npz")))
    shape = {t: (int(gold[f"{t}_full"]), int(gold[f"{t}_B"]), int(gold[f"{t}_K"]), int(gold[f"{t}_G"]), float(gold[f"{t}_lam"]))
             for t in TAGS}
    assert {shape[t] for t in TAGS if t != "d"} == {(0, 2, 4, 2, 1.0), (0, 2, 4, 4, 0.5), (0, 2, 6, 3, 1.0)}
    assert shape["d"] == (1, 1, 4, 2, 1.0)
    runs = [(t, i) for t in TAGS for i in range(int(gold[f"{t}_n"]))]
    assert {float(gold[f"{t}_{i}_lp"]) for t, i in runs} == {0.5, 1.0}
    assert {str(gold[f"{t}_{i}_mode"]) for t, i in runs} == {"4.33", "generated"}
    assert sorted(int(gold[f"a0_{i}_early"]) for i in range(int(gold["a0_n"]))) == [0, 1, 2]
    assert any(json.loads(str(gold[f"{t}_{i}_proc"])) for t, i in runs)
    for t in TAGS:
        if t != "d":
            assert (int(gold[f"{t}_seed"]), float(gold[f"{t}_stop_bias"]), int(gold[f"{t}_Tc"]), int(gold[f"{t}_max_new"]),
                    float(gold[f"{t}_rep"])) == (31, 1.6, 11, 32, 2.0)
    shows = set()
    for t in TAGS:
        shows |= set(gold[f"{t}_shows"].tolist())
    assert {"staggered", "mixed", "diverse"} <= shows


def _tiny_gpt(max_slots=8):
    from genvc_amd.layers.gpt import GPT
    g = GPT(layers=2, model_dim=256, heads=4)
    g.engine = object()                        # (only its presence is checked before the rules below)
    g.max_slots = max_slots
    return g


def test_group_kwarg_rules():
    from genvc_amd.layers.gpt import _beam_groups, _beam_kwargs
    base = dict(num_beams=4, do_sample=False)
    assert _beam_groups(base) == (1, 0.0) and _beam_groups(dict(base, num_beam_groups=1, diversity_penalty=0.0)) == (1, 0.0)
    assert _beam_groups(dict(base, num_beam_groups=2, diversity_penalty=1.0)) == (2, 1.0)
    assert _beam_groups(dict(base, num_beam_groups=4, diversity_penalty=0.5, typical_p=1.0)) == (4, 0.5)
    assert _beam_kwargs(dict(base, num_beam_groups=2, diversity_penalty=1.0, num_return_sequences=4)) == (4, 1.0, 1.0, "4.33")
    g = _tiny_gpt()
    cond, codes = torch.zeros(1, 32, 256), torch.zeros(1, 5, dtype=torch.long)
    grp = dict(base, num_beam_groups=2, diversity_penalty=1.0)
    for kw, match in ((dict(grp, do_sample=True), "do_sample"),
                      (dict(grp, num_beams=6, num_beam_groups=4), "divisible"),
                      (dict(grp, num_beams=2, num_beam_groups=4), "smaller or equal to `num_beams`"),
                      (dict(grp, num_beams=1), "smaller or equal to `num_beams`"),
                      (dict(grp, num_return_sequences=5), "smaller or equal to `num_beams`"),
                      (dict(grp, typical_p=0.5), "typical_p"),
                      (dict(base, diversity_penalty=1.0), "num_beam_groups"),
                      (dict(base, num_beam_groups=1, diversity_penalty=0.5), "num_beam_groups"),
                      (dict(grp, diversity_penalty=-1.0), "diversity_penalty"),
                      (dict(grp, diversity_penalty=float("nan")), "diversity_penalty"),
                      (dict(grp, diversity_penalty=float("inf")), "diversity_penalty"),
                      (dict(grp, num_beam_groups=0), "num_beam_groups")):
        with pytest.raises(ValueError, match=match):
            g.generate(cond, codes, **kw)
    # G > 1 without a positive diversity_penalty: identical groups are not served (tests/test_beam_host.py pins the error type)
    for kw in (dict(base, num_beams=2, num_beam_groups=2), dict(base, num_beam_groups=2, diversity_penalty=0.0)):
        with pytest.raises(NotImplementedError, match="identical groups"):
            g.generate(cond, codes, **kw)
    with pytest.raises(NotImplementedError, match="beam sampling"):            # plain beams with do_sample keep their error
        g.generate(cond, codes, num_beams=4, do_sample=True)
    with pytest.raises(ValueError, match="KV slots"):                          # B * K above the context's slots
        g.generate(torch.zeros(3, 32, 256), torch.zeros(3, 5, dtype=torch.long), **grp)
    with pytest.raises(ValueError, match="contrastive"):                       # contrastive kwargs keep their precedence
        g.generate(cond, codes, top_k=4, penalty_alpha=0.6, num_return_sequences=2, **grp)


def test_paths_that_do_not_serve_groups_raise_through_no_beams():
    from genvc_amd.layers.gpt import GPT
    g = GPT(layers=2, model_dim=256, heads=4)
    cond, codes = torch.zeros(1, 32, 256), torch.zeros(1, 5, dtype=torch.long)
    kw = dict(num_beams=4, do_sample=False, num_beam_groups=2, diversity_penalty=1.0)
    with pytest.raises(NotImplementedError, match=re.escape("streaming (get_generator)")):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))
    with pytest.raises(NotImplementedError, match=re.escape("grouped (generate_groups)")):
        g.generate_groups([(cond, codes)], **kw)
    with pytest.raises(NotImplementedError, match=re.escape("rolling (generate_rolling)")):
        g.generate_rolling([(cond, codes)], **kw)


def test_group_symbols_declared_and_exported_and_the_state_keeps_its_size():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    assert "gvc_beam_groups" in hdr
    assert ctypes.sizeof(_lib.BeamState) == 10 * 4 + 12 * 8
    assert ctypes.sizeof(_lib.BeamGroups) == 2 * 4 + 3 * 8
    assert [f for f, _ in _lib.BeamGroups._fields_] == ["G", "diversity_penalty", "done", "hyp_count", "hyp_worst"]
    m = re.search(r"typedef struct \{\s*int32_t G;[^}]*float diversity_penalty;[^}]*int32_t\* done;[^}]*int32_t\* hyp_count;[^}]*"
                  r"float\* hyp_worst;[^}]*\} gvc_beam_groups;", hdr)
    assert m
    if os.path.exists(_lib.LIB_PATH):
        import subprocess
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s
