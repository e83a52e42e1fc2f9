"""CPU: the N-best / early_stopping restatement (tests/nbest_oracle.py) against the executed reference (tests/golden/nbest.npz,
scripts/make_nbest_golden.py), the kwarg rules of num_return_sequences on every path, and the new C ABI symbols."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402
import nbest_oracle as NO                     # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "nbest.npz")
SYMBOLS = ("gvc_gpt_kv_fanout", "gvc_gpt_sequence_logprobs")


def runs(gold, tag):
    for i in range(int(gold[f"{tag}_n"])):
        p = f"{tag}_{i}_"
        yield p, int(gold[p + "N"]), float(gold[p + "lp"]), NO.EARLY[int(gold[p + "early"])]


@pytest.mark.parametrize("tag", NO.TAGS)
def test_restatement_reproduces_the_executed_reference(tag):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gold = dict(np.load(GOLD))
    margs = gcfg.DEFAULT_MODEL_ARGS if int(gold[f"{tag}_full"]) else gcfg.TINY_MODEL_ARGS
    dims = gcfg.gpt_dims(margs)
    w = synth.make_weights(int(gold[f"{tag}_seed"]), synth.gpt_weight_spec(dims))
    if float(gold[f"{tag}_stop_bias"]) != 0.0:
        w["mel_head.bias"][1025] = float(gold[f"{tag}_stop_bias"])
    ora = BO.OracleGpt(w, dims)
    B, Tc, s, K = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"]), int(gold[f"{tag}_K"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (B, Tc), 256)
    for p, N, lp, early in runs(gold, tag):
        r = NO.beam_search(ora, cond, codes, K, lp, float(gold[f"{tag}_rep"]), int(gold[f"{tag}_max_new"]), mode="generated",
                           early_stopping=early, num_return=N)
        assert r["ids"].shape == gold[p + "ids"].shape and np.array_equal(r["ids"], gold[p + "ids"]), (p, N, lp, early)
        assert gold[p + "ids"].shape[0] == B * N
        np.testing.assert_allclose(r["scores"], gold[p + "scores"], rtol=1e-5)
        # both screens hold, stored and recomputed
        assert r["min_gap"] >= 1e-3 and float(gold[p + "min_gap"]) >= 1e-3
        assert r["order_gap"] >= 1e-3 and float(gold[p + "order_gap"]) >= 1e-3
        # best first; row 0 of every item is the num_return_sequences = 1 result
        sc = r["scores"].reshape(B, N)
        assert bool((sc[:, :-1] > sc[:, 1:]).all())
        one = NO.beam_search(ora, cond, codes, K, lp, float(gold[f"{tag}_rep"]), int(gold[f"{tag}_max_new"]), mode="generated",
                             early_stopping=early, num_return=1)
        w1 = min(one["ids"].shape[1], r["ids"].shape[1])
        assert np.array_equal(one["ids"][:, :w1], r["ids"][::N, :w1])
        if early is False:
            base = BO.beam_search(ora, cond, codes, K, lp, float(gold[f"{tag}_rep"]), int(gold[f"{tag}_max_new"]), mode="generated")
            assert np.array_equal(base["ids"], one["ids"])                    # ... which is tests/beam_oracle.py's


def test_fixture_cases_cover_the_issue():
    gold = dict(np.load(GOLD))
    shape = {t: (int(gold[f"{t}_full"]), int(gold[f"{t}_B"]), int(gold[f"{t}_K"])) for t in NO.TAGS}
    assert all(shape[t] == (0, 3, 3) for t in ("a0", "a1", "a2")) and all(shape[t] == (0, 2, 4) for t in ("b0", "b1"))
    assert shape["c"] == (1, 1, 4)
    seen = {t: sorted({(N, lp) for _, N, lp, _ in runs(gold, t)}) for t in NO.TAGS}
    assert {N for t in ("a0", "a1", "a2") for N, _ in seen[t]} == {2, 3}
    assert {N for t in ("b0", "b1") for N, _ in seen[t]} == {2} and seen["c"] == [(4, 1.0)]
    assert {lp for t in NO.TAGS for _, lp in seen[t]} == {0.5, 1.0, 2.0}
    true_differs = never_differs = ragged = False
    for t in NO.TAGS:
        by = {(N, lp, str(e)): gold[p + "ids"] for p, N, lp, e in runs(gold, t)}
        assert len(by) == 3 * len(seen[t])                                    # every (N, lp) under the three early_stopping modes
        for N, lp in seen[t]:
            f, tr, nv = by[(N, lp, "False")], by[(N, lp, "True")], by[(N, lp, "never")]
            true_differs |= f.shape != tr.shape or not np.array_equal(f, tr)
            never_differs |= lp > 0 and (f.shape != nv.shape or not np.array_equal(f, nv))
        for ids in by.values():
            ends = {int((row == 1025).argmax()) if (row == 1025).any() else ids.shape[1] for row in ids}
            ragged |= len(ends) > 1
    assert true_differs and never_differs and ragged


def _tiny_gpt(max_slots=8):
    from genvc_amd.layers.gpt import GPT
    g = GPT(layers=2, model_dim=256, heads=4)
    g.engine = object()                        # (only its presence is checked before the rules below)
    g.max_slots = max_slots
    return g


def test_beam_kwarg_rules():
    from genvc_amd.engine import beam_early_stopping
    from genvc_amd.layers.gpt import _beam_kwargs, _beam_returns
    beam = dict(num_beams=4, do_sample=False)
    assert _beam_kwargs(dict(beam, num_return_sequences=2, early_stopping=True)) == (4, 1.0, 1.0, "4.33")
    assert _beam_returns(dict(beam, num_return_sequences=4, early_stopping="never")) == (4, "never")
    assert _beam_returns(beam) == (1, False)
    assert [beam_early_stopping(v) for v in (False, True, "never")] == [0, 1, 2]
    with pytest.raises(ValueError, match="smaller or equal to `num_beams`"):
        _beam_kwargs(dict(beam, num_return_sequences=5))
    with pytest.raises(ValueError, match="at least 1"):
        _beam_kwargs(dict(beam, num_return_sequences=0))
    for bad in ("always", 1, None, 0):
        with pytest.raises(ValueError, match="early_stopping"):
            _beam_kwargs(dict(beam, early_stopping=bad))
    g = _tiny_gpt()
    cond, codes = torch.zeros(1, 32, 256), torch.zeros(1, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="smaller or equal"):
        g.generate(cond, codes, num_return_sequences=3, num_beams=2, do_sample=False)
    with pytest.raises(NotImplementedError, match="beam sampling"):            # still out of scope, whatever N
        g.generate(cond, codes, num_return_sequences=2, num_beams=2, do_sample=True)


def test_beam_state_keeps_its_size_and_packs_the_mode():
    """early_stopping travels in bits 8..15 of gvc_beam_state.length_mode: the struct keeps its layout, and a positional construction
    that sets the length mode alone gets early_stopping=False"""
    import ctypes
    from genvc_amd import _lib
    assert ctypes.sizeof(_lib.BeamState) == 10 * 4 + 12 * 8
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    assert re.search(r"int32_t length_mode;\s*/\* bits 0\.\.7: .* bits 8\.\.15: early_stopping", hdr)
    import inspect
    from genvc_amd.engine import BeamSearch
    params = list(inspect.signature(BeamSearch.__init__).parameters)
    assert params[-1] == "early_stopping" and params[1:10] == ["fake", "K", "max_new", "eos", "vocab", "length_penalty",
                                                               "repetition_penalty", "length_mode", "proc"]
    assert inspect.signature(BeamSearch.__init__).parameters["early_stopping"].default is False


def test_sampling_kwarg_rules():
    from genvc_amd.layers.gpt import _sample_return_kwargs
    assert _sample_return_kwargs({}) == 1 and _sample_return_kwargs(dict(num_return_sequences=None)) == 1
    assert _sample_return_kwargs(dict(num_return_sequences=4, do_sample=True), B=2, max_slots=8) == 4
    assert _sample_return_kwargs(dict(num_return_sequences=4)) == 4                   # (this build's generate samples by default)
    with pytest.raises(ValueError, match=r"init_gpt_for_inference\(max_slots"):
        _sample_return_kwargs(dict(num_return_sequences=3), B=3, max_slots=8)
    with pytest.raises(ValueError, match="greedy"):
        _sample_return_kwargs(dict(num_return_sequences=2, do_sample=False))
    with pytest.raises(ValueError, match="at least 1"):
        _sample_return_kwargs(dict(num_return_sequences=0))
    g = _tiny_gpt()
    cond, codes = torch.zeros(3, 32, 256), torch.zeros(3, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="KV slots"):
        g.generate(cond, codes, do_sample=True, num_return_sequences=3)
    with pytest.raises(ValueError, match="greedy"):
        g.generate(cond, codes, do_sample=False, num_return_sequences=2)
    with pytest.raises(ValueError, match="at least 1"):
        g.generate(cond, codes, num_return_sequences=-1)
    with pytest.raises(ValueError, match="contrastive"):                       # keeps its own error
        g.generate(cond[:1], codes[:1], do_sample=False, top_k=4, penalty_alpha=0.6, num_return_sequences=2)


def test_paths_that_do_not_serve_it_name_themselves():
    from genvc_amd.layers.gpt import GPT
    g = GPT(layers=2, model_dim=256, heads=4)
    cond, codes = torch.zeros(1, 32, 256), torch.zeros(1, 5, dtype=torch.long)
    kw = dict(num_return_sequences=2)
    with pytest.raises(NotImplementedError, match=re.escape("streaming (get_generator)")):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))
    with pytest.raises(NotImplementedError, match=re.escape("grouped (generate_groups)")):
        g.generate_groups([(cond, codes)], **kw)
    with pytest.raises(NotImplementedError, match=re.escape("rolling (generate_rolling)")):
        g.generate_rolling([(cond, codes)], **kw)
    # the harness's explicit num_return_sequences=1 passes the rule (and reaches the engine check of this CPU-only module)
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), num_return_sequences=1))
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
        g.generate_groups([(cond, codes)], num_return_sequences=1)


def test_new_symbols_declared_and_exported():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    if os.path.exists(_lib.LIB_PATH):
        import subprocess
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s
