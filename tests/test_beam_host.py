"""CPU: the beam-search restatement (tests/beam_oracle.py) against the executed reference (tests/golden/beam_search.npz), the modes
that keep raising NotImplementedError, and the new C ABI symbols."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "beam_search.npz")
SYMBOLS = ("gvc_beam_select", "gvc_gpt_beam_generate", "gvc_gpt_warmup_beam")


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_reproduces_the_executed_reference(tag):
    gold = dict(np.load(GOLD))
    margs = gcfg.DEFAULT_MODEL_ARGS if int(gold[f"{tag}_full"]) else gcfg.TINY_MODEL_ARGS
    dims = gcfg.gpt_dims(margs)
    w = synth.make_weights(int(gold[f"{tag}_seed"]), synth.gpt_weight_spec(dims))
    if float(gold[f"{tag}_stop_bias"]) != 0.0:
        w["mel_head.bias"][1025] = float(gold[f"{tag}_stop_bias"])
    ora = BO.OracleGpt(w, dims)
    B, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (B, Tc), 256)
    outs = []
    for i in range(int(gold[f"{tag}_n"])):
        r = BO.beam_search(ora, cond, codes, int(gold[f"{tag}_K"]), float(gold[f"{tag}_{i}_lp"]), float(gold[f"{tag}_rep"]),
                           int(gold[f"{tag}_max_new"]), mode="generated")
        assert np.array_equal(r["ids"], gold[f"{tag}_{i}_ids"])
        np.testing.assert_allclose(r["best_scores"], gold[f"{tag}_{i}_best_scores"], rtol=1e-5)
        assert r["min_gap"] >= 1e-3 and float(gold[f"{tag}_{i}_min_gap"]) >= 1e-3       # the margin screen holds
        outs.append(gold[f"{tag}_{i}_ids"])
    if tag == "b":
        # the case is built to matter: rows end at different steps, and the winner depends on length_penalty
        ends = [(o == 1025).argmax(1) for o in outs]
        assert any(len(set(e.tolist())) > 1 for e in ends)
        assert len({o.tobytes() for o in outs}) > 1


def test_length_modes_differ_where_lengths_matter():
    """the two length modes are one integer each: with n0 + t vs t + 1 the normalised scores differ"""
    assert BO.norm_len("4.33", 44, 3) == 47 and BO.norm_len("generated", 44, 3) == 4


def _tiny_gpt():
    from genvc_amd.layers.gpt import GPT
    return GPT(layers=2, model_dim=256, heads=4)


@pytest.mark.parametrize("call", ["sample", "groups", "rolling", "generator", "groups_beam_kw"])
def test_out_of_scope_beam_modes_raise(call):
    g = _tiny_gpt()
    cond, codes = torch.zeros(1, 32, 256), torch.zeros(1, 5, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="beam"):
        if call == "sample":
            g.generate(cond, codes, num_beams=4, do_sample=True)
        elif call == "groups":
            g.generate_groups([(cond, codes)], num_beams=2, do_sample=False)
        elif call == "rolling":
            g.generate_rolling([(cond, codes)], num_beams=2, do_sample=False)
        elif call == "generator":
            next(g.get_generator(torch.ones(1, 8, dtype=torch.long), num_beams=3, do_sample=False))
        else:
            g.generate(cond, codes, num_beams=2, do_sample=False, num_beam_groups=2)


def test_beam_width_beyond_the_slots_is_a_value_error():
    g = _tiny_gpt()
    g.engine = object()                        # (only its presence is checked before the slot bound)
    g.max_slots = 8
    with pytest.raises(ValueError, match="KV slots"):
        g.generate(torch.zeros(3, 32, 256), torch.zeros(3, 5, dtype=torch.long), num_beams=4, do_sample=False)


def test_beam_symbols_are_declared_and_exported():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\bint " + s + r"\(", hdr), s
        assert s in _lib.exported_symbols(), s
    assert "gvc_beam_state" in hdr
    import ctypes
    assert ctypes.sizeof(_lib.BeamState) == 10 * 4 + 12 * 8
