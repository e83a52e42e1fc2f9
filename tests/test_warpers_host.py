"""CPU: the typical / epsilon / eta sampling warpers -- the restatement (tests/warp_oracle.py) against the installed transformers' classes,
on / off / ValueError behaviour, packing and validation of the kwargs, the C ABI's struct and symbols, the infer.py flags and the
executed-reference fixture (tests/golden/logits_warpers.npz, scripts/make_warper_golden.py)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import warp_oracle as WO      # noqa: E402
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
import beam_oracle as BO                  # noqa: E402

GOLD = os.path.join(HERE, "golden", "logits_warpers.npz")
V, EOS = 1026, 1025
SYMBOLS = ("gvc_sample_warp", "gvc_gpt_generate_warp")


def _rows(seed, n=24):
    """random score rows with -inf entries (earlier warpers' masks) and tied values"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        s = torch.randn(V, generator=g) * (0.5 + 3.0 * torch.rand(1, generator=g))
        if i % 3 == 0:
            s[torch.randperm(V, generator=g)[:V // 2]] = -float("inf")
        if i % 4 == 1:
            s[torch.randperm(V, generator=g)[:V - 40]] = -float("inf")        # a top-k-like row: 40 survivors
        if i % 2 == 0:
            idx = torch.randperm(V, generator=g)[:60]
            s[idx[30:]] = s[idx[:30]]                                          # ties
        out.append(s)
    return out


def _hf(cls, v):
    from transformers.generation import logits_process as LP
    return getattr(LP, cls)(v)


@pytest.mark.parametrize("mass", [0.05, 0.2, 0.5, 0.9, 0.99])
def test_typical_restatement_equals_installed_transformers(mass):
    for s in _rows(1):
        ref = torch.isfinite(_hf("TypicalLogitsWarper", mass)(None, s[None])[0])
        assert torch.equal(WO.typical_keep(s, mass), ref)


@pytest.mark.parametrize("eps", [1e-4, 3e-3, 0.02, 0.2, 0.6])
def test_cutoff_restatements_equal_installed_transformers(eps):
    for s in _rows(2):
        assert torch.equal(WO.epsilon_keep(s, eps), torch.isfinite(_hf("EpsilonLogitsWarper", eps)(None, s[None])[0]))
        assert torch.equal(WO.eta_keep(s, eps), torch.isfinite(_hf("EtaLogitsWarper", eps)(None, s[None])[0]))


def test_typical_ties_and_argmax():
    """tied keys are kept together, whatever the order inside the tie, and typical can drop the argmax"""
    s = torch.full((V,), -float("inf"))
    s[:6] = torch.tensor([3.0, 1.0, 1.0, 0.9, 0.9, -2.0])
    keep = WO.typical_keep(s, 0.3)
    assert keep[1] == keep[2] and keep[3] == keep[4]
    ref = torch.isfinite(_hf("TypicalLogitsWarper", 0.3)(None, s[None])[0])
    assert torch.equal(keep, ref)
    s2 = torch.full((V,), -float("inf"))
    s2[:12] = torch.tensor([2.0] + [0.0] * 11)          # one dominant id: its surprisal is far from the entropy of this shape
    k2 = WO.typical_keep(s2, 0.3)
    assert torch.equal(k2, torch.isfinite(_hf("TypicalLogitsWarper", 0.3)(None, s2[None])[0]))
    assert not bool(k2[0])


def test_warp_order_is_the_installed_one():
    from transformers import GenerationConfig, GenerationMixin
    cfg = GenerationConfig(do_sample=True, top_k=15, top_p=0.85, temperature=0.75, min_p=0.05, typical_p=0.5, epsilon_cutoff=0.1,
                           eta_cutoff=0.2)

    class _M:
        config = type("C", (), {"is_encoder_decoder": False})()
        _merge_criteria_processor_list = GenerationMixin._merge_criteria_processor_list
    names = [type(p).__name__ for p in GenerationMixin._get_logits_processor(_M(), generation_config=cfg, input_ids_seq_length=4,
                                                                              encoder_input_ids=None, logits_processor=None, device="cpu")]
    order = ["TemperatureLogitsWarper", "TopKLogitsWarper", "TopPLogitsWarper", "MinPLogitsWarper", "TypicalLogitsWarper",
             "EpsilonLogitsWarper", "EtaLogitsWarper"]
    assert [n for n in names if n in order] == order


GRID = [None, -1.0, -0.0, 0.0, 1e-9, 0.3, 0.999, 1.0, 1.5, float("nan"), float("inf"), 3]


def _installed(kw, do_sample=True):
    """which of the three transformers builds for these kwargs -> {name: value} (or the exception type it raises)"""
    from transformers import GenerationConfig, GenerationMixin

    class _M:
        config = type("C", (), {"is_encoder_decoder": False})()
        _merge_criteria_processor_list = GenerationMixin._merge_criteria_processor_list
    try:
        cfg = GenerationConfig(do_sample=do_sample, top_k=None, top_p=None, temperature=None, **kw)
        ps = GenerationMixin._get_logits_processor(_M(), generation_config=cfg, input_ids_seq_length=4, encoder_input_ids=None,
                                                   logits_processor=None, device="cpu")
    except ValueError:
        return ValueError
    out = {}
    for p in ps:
        n = type(p).__name__
        if n == "TypicalLogitsWarper":
            out["typical_p"] = p.mass
        elif n == "EpsilonLogitsWarper":
            out["epsilon_cutoff"] = p.epsilon
        elif n == "EtaLogitsWarper":
            out["eta_cutoff"] = float(p.epsilon)
    return out


@pytest.mark.parametrize("name", WO.KEYS)
@pytest.mark.parametrize("do_sample", [True, False])
def test_on_off_and_errors_match_installed_transformers(name, do_sample):
    from genvc_amd.engine import logits_warpers
    for v in GRID:
        kw = {name: v}
        want = _installed(kw, do_sample)
        if want is ValueError:
            with pytest.raises(ValueError):
                logits_warpers(kw, sampling=do_sample)
            continue
        w = logits_warpers(kw, sampling=do_sample)
        if not want:
            assert w is None, (name, v)
        else:
            assert w is not None and getattr(w, name) == pytest.approx(want[name], rel=1e-6), (name, v)
            assert [k for k in WO.KEYS if getattr(w, k) != 0.0] == [name]
        # the restatement's rule agrees
        if do_sample:
            assert [k for k, _ in WO.on_values(kw)] == list(want)


def test_packing_defaults_and_validation():
    from genvc_amd.engine import logits_warpers
    assert logits_warpers({}) is None
    assert logits_warpers(dict(typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)) is None
    assert logits_warpers(dict(typical_p=0.4, epsilon_cutoff=3e-4), sampling=False) is None
    w = logits_warpers(dict(typical_p=0.4, epsilon_cutoff=3e-4, eta_cutoff=2e-3, min_new_tokens=3))
    assert (w.typical_p, w.epsilon_cutoff, w.eta_cutoff, w.reserved) == pytest.approx((0.4, 3e-4, 2e-3, 0))
    # on values stay inside (0, 1) in float32 (0 is "off" on the device)
    assert 0.0 < logits_warpers(dict(epsilon_cutoff=1e-60)).epsilon_cutoff < 1e-30
    assert logits_warpers(dict(typical_p=1.0 - 1e-12)).typical_p < 1.0
    for bad in (dict(typical_p=0.0), dict(typical_p=-0.5), dict(typical_p="x"), dict(eta_cutoff=[0.1]), dict(epsilon_cutoff=True)):
        with pytest.raises(ValueError):
            logits_warpers(bad)


def test_struct_layout_and_symbols():
    from genvc_amd import _lib
    assert C.sizeof(_lib.LogitsWarpers) == 16
    assert [f for f, _ in _lib.LogitsWarpers._fields_] == ["typical_p", "epsilon_cutoff", "eta_cutoff", "reserved"]
    assert C.sizeof(_lib.LogitsProcessors) == 48 + 2 * 33 * 4 and C.sizeof(_lib.RowSampling) == 32      # unchanged
    header = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    assert re.search(r"typedef struct gvc_logits_warpers \{\s*float typical_p;[^}]*float epsilon_cutoff;[^}]*float eta_cutoff;"
                     r"[^}]*int32_t reserved;[^}]*\} gvc_logits_warpers;", header)
    declared = set(re.findall(r"\b(gvc_[a-z0-9_]+)\s*\(", header))
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.exported_symbols(), s


def test_per_item_dicts_accept_warpers_and_reject_others():
    from genvc_amd.engine import WARP_KWARGS, check_proc_kwargs
    check_proc_kwargs(dict(typical_p=0.5, epsilon_cutoff=3e-4, eta_cutoff=1e-3, min_p=0.1), "row 0")
    assert set(WARP_KWARGS) == set(WO.KEYS)
    with pytest.raises(ValueError, match="'top_k' is not a processor kwarg"):
        check_proc_kwargs(dict(typical_p=0.5, top_k=3), "group_kwargs[1]")
    with pytest.raises(ValueError, match="'top_h' is not a processor kwarg"):
        check_proc_kwargs(dict(top_h=0.3), "row 2")


def test_logits_sets_pairs_processors_with_warpers():
    from genvc_amd.engine import ProcessorSets, WarperSets, logits_processor_sets, logits_sets
    kws = [dict(min_new_tokens=3), None, dict(min_new_tokens=3, typical_p=0.5), dict(typical_p=0.5), dict(min_new_tokens=3, typical_p=0.5),
           dict(eta_cutoff=2.0)]
    ws = logits_sets(kws, 10, V)
    assert isinstance(ws, WarperSets)
    assert list(ws.set_of_row) == [0, -1, 1, 2, 1, -1]           # (eta_cutoff 2 is off: that row has neither)
    assert ws.n_sets == 3 and ws.sets is not None
    assert ws.sets[0].min_new_tokens == 3 and ws.sets[2].min_new_tokens == 0
    assert ws.warps[0].typical_p == 0.0 and ws.warps[1].typical_p == pytest.approx(0.5)
    # no warper on anywhere: exactly logits_processor_sets()
    plain = [dict(min_new_tokens=3), None, dict(min_new_tokens=3, eta_cutoff=0.0)]
    a, b = logits_sets(plain, 10, V), logits_processor_sets(plain, 10, V)
    assert isinstance(a, ProcessorSets) and list(a.set_of_row) == list(b.set_of_row) and a.n_sets == b.n_sets
    assert logits_sets([None, dict(typical_p=0.3)], 10, V, sampling=False) is None
    only = logits_sets([dict(epsilon_cutoff=0.1), None], 10, V)
    assert only.sets is None and list(only.set_of_row) == [0, -1]
    with pytest.raises(ValueError, match="row 1"):
        logits_sets([None, dict(typical_p=-1.0)], 10, V)
    one = WarperSets.one(None, ws.warps[1], 5)
    assert list(one.set_of_row) == [0] * 5 and one.sets is None


@pytest.mark.parametrize("flags", [["--typical_p", "0"], ["--typical_p", "-0.2"], ["--typical_p", "1.5"], ["--epsilon_cutoff", "1"],
                                   ["--eta_cutoff", "-0.1"], ["--eta_cutoff", "x"]])
def test_infer_rejects_malformed_flags(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--synthetic", "--device", "cpu"] + flags, capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0
    assert "bad warper flag" in r.stderr or "bad processor flag" in r.stderr or "error:" in r.stderr, r.stderr[-500:]


# ------------------------------------------------------------------------------------------------------------------------------
# the executed-reference fixture

def _cases():
    return json.loads(str(np.load(GOLD)["cases"]))


def case_inputs(gold, tag):
    """(oracle GPT, cond, codes, warper kwargs, sampling settings) of a fixture case"""
    margs = gcfg.DEFAULT_MODEL_ARGS if int(gold[f"{tag}_full"]) else gcfg.TINY_MODEL_ARGS
    dims = gcfg.gpt_dims(margs)
    w = synth.make_weights(int(gold[f"{tag}_seed"]), synth.gpt_weight_spec(dims))
    B, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (B, Tc), 256)
    return BO.OracleGpt(w, dims), cond, codes, json.loads(str(gold[f"{tag}_kw"])), json.loads(str(gold[f"{tag}_samp"]))


def test_fixture_covers_each_warper_sizes_and_the_harness_settings():
    gold = dict(np.load(GOLD))
    cases = _cases()
    kws = [json.loads(str(gold[f"{t}_kw"])) for t in cases]
    for k in WO.KEYS:
        assert {k} in [set(kw) for kw in kws], k                        # each warper alone
    assert {int(gold[f"{t}_full"]) for t in cases} == {0, 1}
    harness = [t for t in cases if json.loads(str(gold[f"{t}_samp"])) == dict(top_k=15, top_p=0.85, temperature=0.75,
                                                                                 repetition_penalty=10.0)]
    assert harness and any(len(json.loads(str(gold[f"{t}_kw"]))) > 1 for t in harness)
    for t in cases:
        # every case was built to matter: its ids differ from the same run without the warpers
        assert gold[f"{t}_tokens"].shape != gold[f"{t}_base"].shape or not np.array_equal(gold[f"{t}_tokens"], gold[f"{t}_base"])
    # typical cases keep an id that is not the argmax at some step
    for t in cases:
        if "typical_p" in json.loads(str(gold[f"{t}_kw"])):
            assert (gold[f"{t}_tokens"] != gold[f"{t}_argmax"]).any(), t


@pytest.mark.parametrize("tag", _cases())
def test_restatement_reproduces_the_executed_reference(tag):
    gold = dict(np.load(GOLD))
    ora, cond, codes, kw, samp = case_inputs(gold, tag)
    toks, marg, amax = WO.single_survivor(ora, cond, codes, kw, samp, int(gold[f"{tag}_max_new"]))
    assert np.array_equal(toks, gold[f"{tag}_tokens"])
    assert np.array_equal(amax, gold[f"{tag}_argmax"])
    # the screens hold: one survivor at every step, margins >= 2e-3
    assert (marg[..., 0] == 1).all()
    assert marg[..., 1:].min() >= 2e-3
