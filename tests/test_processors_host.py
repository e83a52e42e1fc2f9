"""CPU: the length / repetition logits processors (include/genvc_hip.h: gvc_logits_processors).  The restatement (tests/proc_oracle.py)
against the installed transformers' classes, the restatement against the executed reference (tests/golden/logits_processors.npz,
scripts/make_processor_golden.py), the host-side packing and validation, the new C ABI symbols and infer.py's flags."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402
import proc_oracle as PO                      # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "logits_processors.npz")
SYMBOLS = ("gvc_sample_proc", "gvc_gpt_generate_proc", "gvc_beam_select_proc", "gvc_gpt_beam_generate_proc")
EOS, V = 1025, 1026


def _rows(gen, B, n0, n_gen):
    """fake prompt rows (n0 - 1 ones, then 1024) followed by generated ids drawn from a small alphabet (so n-grams repeat)"""
    rows = []
    for _ in range(B):
        tail = torch.randint(0, 6, (n_gen,), generator=gen) * 150
        rows.append([1] * (n0 - 1) + [1024] + tail.tolist())
    return rows


CASES = [
    dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2), dict(no_repeat_ngram_size=3), dict(no_repeat_ngram_size=8),
    dict(min_length=60), dict(min_length=10), dict(min_new_tokens=5), dict(min_new_tokens=40),
    dict(exponential_decay_length_penalty=(3, 1.7)), dict(exponential_decay_length_penalty=(-2, 0.8)),
    dict(suppress_tokens=[0, 5, 1025]), dict(begin_suppress_tokens=[7, 1025]),
    dict(no_repeat_ngram_size=2, min_new_tokens=3, suppress_tokens=[300], begin_suppress_tokens=[1025],
         exponential_decay_length_penalty=(20, 1.2)),
]


@pytest.mark.parametrize("kw", CASES, ids=[json.dumps(c) for c in CASES])
@pytest.mark.parametrize("n_gen", [0, 1, 7, 30])
def test_restatement_equals_installed_transformers(kw, n_gen):
    gen = torch.Generator().manual_seed(17 + n_gen + 1000 * CASES.index(kw))
    B, n0 = 3, 12
    rows = _rows(gen, B, n0, n_gen)
    ids = torch.tensor(rows)
    scores = torch.randn(B, V, generator=gen) * 4.0
    procs = PO.hf_processors(kw, n0, EOS)
    names = [type(p).__name__ for p in procs]
    assert "RepetitionPenaltyLogitsProcessor" not in names and len(names) >= 1
    want = scores.clone()
    for p in procs:
        want = p(ids, want)
    got = torch.stack([PO.process(scores[b], rows[b], n0, kw, EOS) for b in range(B)])
    assert torch.equal(torch.isinf(got), torch.isinf(want))
    assert torch.equal(got, want), (got - want).abs().max()


def test_processor_order_is_the_installed_one():
    kw = dict(no_repeat_ngram_size=2, min_length=5, min_new_tokens=3, exponential_decay_length_penalty=(4, 1.1), suppress_tokens=[3],
              begin_suppress_tokens=[4], min_p=0.1)
    names = [type(p).__name__ for p in PO.hf_processors(kw, 9, EOS, sampling=True)]
    assert names == ["NoRepeatNGramLogitsProcessor", "MinLengthLogitsProcessor", "MinNewTokensLengthLogitsProcessor",
                     "ExponentialDecayLengthPenalty", "SuppressTokensLogitsProcessor", "SuppressTokensAtBeginLogitsProcessor",
                     "MinPLogitsWarper"]


@pytest.mark.parametrize("min_p", [0.02, 0.2, 0.7])
def test_min_p_restatement_equals_installed_transformers(min_p):
    from transformers.generation.logits_process import MinPLogitsWarper
    gen = torch.Generator().manual_seed(int(min_p * 1000))
    s = torch.randn(4, V, generator=gen) * 3.0
    want = MinPLogitsWarper(min_p)(None, s.clone())
    for b in range(4):
        keep = PO.min_p_keep(s[b], min_p)
        assert torch.equal(keep, want[b] > -float("inf"))


def _case(gold, tag):
    margs = gcfg.DEFAULT_MODEL_ARGS if int(gold[f"{tag}_full"]) else gcfg.TINY_MODEL_ARGS
    dims = gcfg.gpt_dims(margs)
    w = synth.make_weights(int(gold[f"{tag}_seed"]), synth.gpt_weight_spec(dims))
    if float(gold[f"{tag}_stop_bias"]) != 0.0:
        w["mel_head.bias"][EOS] = float(gold[f"{tag}_stop_bias"])
    B, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (B, Tc), 256)
    kw = json.loads(str(gold[f"{tag}_kw"]))
    if "exponential_decay_length_penalty" in kw:
        kw["exponential_decay_length_penalty"] = tuple(kw["exponential_decay_length_penalty"])
    return BO.OracleGpt(w, dims), cond, codes, kw


def _cases():
    return json.loads(str(np.load(GOLD)["cases"]))


def test_fixture_has_tiny_full_sampler_and_beam_cases():
    gold = dict(np.load(GOLD))
    cases = _cases()
    kinds = {str(gold[f"{t}_kind"]) for t in cases}
    assert kinds == {"sampler", "beam"}
    assert {int(gold[f"{t}_full"]) for t in cases} == {0, 1}
    keys = set()
    for t in cases:
        keys |= set(json.loads(str(gold[f"{t}_kw"])))
        # every case was built to matter: its ids differ from the same run without the processors
        assert gold[f"{t}_tokens"].shape != gold[f"{t}_base"].shape or not np.array_equal(gold[f"{t}_tokens"], gold[f"{t}_base"])
    assert keys == set(PO.KEYS) - {"min_p"}


@pytest.mark.parametrize("tag", _cases())
def test_restatement_reproduces_the_executed_reference(tag):
    gold = dict(np.load(GOLD))
    ora, cond, codes, kw = _case(gold, tag)
    max_new = int(gold[f"{tag}_max_new"])
    if str(gold[f"{tag}_kind"]) == "sampler":
        toks, gaps = PO.greedy(ora, cond, codes, kw, float(gold[f"{tag}_rep"]), max_new)
        assert np.array_equal(toks, gold[f"{tag}_tokens"])
        assert np.isfinite(gaps).sum() and gaps[np.isfinite(gaps)].min() >= 2e-3           # the margin screen holds
    else:
        r = PO.beams(ora, cond, codes, int(gold[f"{tag}_K"]), float(gold[f"{tag}_lp"]), float(gold[f"{tag}_rep"]), max_new, kw)
        assert np.array_equal(r["ids"], gold[f"{tag}_tokens"])
        np.testing.assert_allclose(r["best_scores"], gold[f"{tag}_best_scores"], rtol=1e-5)
        assert r["min_gap"] >= 1e-3


@pytest.mark.parametrize("tag", _cases())
def test_every_processor_of_a_case_matters(tag):
    """each kwarg a fixture case sets changes its ids on its own: without it (the others kept) the restatement gives other ids"""
    gold = dict(np.load(GOLD))
    ora, cond, codes, kw = _case(gold, tag)
    max_new, rep = int(gold[f"{tag}_max_new"]), float(gold[f"{tag}_rep"])
    want = gold[f"{tag}_tokens"]
    for k in kw:
        rest = {j: v for j, v in kw.items() if j != k}
        if str(gold[f"{tag}_kind"]) == "sampler":
            got, _ = PO.greedy(ora, cond, codes, rest, rep, max_new)
        else:
            got = PO.beams(ora, cond, codes, int(gold[f"{tag}_K"]), float(gold[f"{tag}_lp"]), rep, max_new, rest)["ids"]
        assert got.shape != want.shape or not np.array_equal(got, want), f"{tag}: {k} does not change the ids"


def test_ngram_cases_repeat_without_the_ban():
    """the n-gram cases are built on runs that repeat: their baseline holds an n-gram twice (counting the fake prompt, as HF does)"""
    gold = dict(np.load(GOLD))
    hit = {"sampler": 0, "beam": 0}
    for tag in _cases():
        n = json.loads(str(gold[f"{tag}_kw"])).get("no_repeat_ngram_size")
        if not n:
            continue
        B, Tc = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"])
        fake = [1] * (32 + Tc + 2) + [1024]
        for r in gold[f"{tag}_base"]:
            row = fake + [int(x) for x in r]
            grams = [tuple(row[i:i + n]) for i in range(len(row) - n + 1) if 1025 not in row[i:i + n]]
            gen = [tuple(row[i:i + n]) for i in range(len(fake) - n + 1, len(row) - n + 1) if 1025 not in row[i:i + n]]
            if any(grams.count(x) > 1 for x in gen):
                hit[str(gold[f"{tag}_kind"])] += 1
                break
    assert hit["sampler"] >= 2 and hit["beam"] >= 2, hit


def test_decay_overlap_deviation_is_the_documented_one():
    """min_new_tokens bans EOS while the decay applies: HF's classes give NaN for EOS, the restatement (and the device) keep -inf"""
    n0 = 10
    row = [1] * (n0 - 1) + [1024] + [5, 6]
    kw = dict(min_new_tokens=4, exponential_decay_length_penalty=(0, 1.5))
    s = torch.randn(V, generator=torch.Generator().manual_seed(1))
    want = s[None].clone()
    for p in PO.hf_processors(kw, n0, EOS):
        want = p(torch.tensor([row]), want)
    assert torch.isnan(want[0, EOS])
    got = PO.process(s, row, n0, kw, EOS)
    assert got[EOS] == -float("inf")
    assert torch.equal(got[:EOS], want[0, :EOS])


def test_packing_defaults_and_validation():
    from genvc_amd.engine import logits_processors
    assert logits_processors({}, 10, V) is None
    assert logits_processors(dict(min_new_tokens=0, min_length=None, no_repeat_ngram_size=0, suppress_tokens=[], min_p=0.0), 10, V) is None
    assert logits_processors(dict(min_p=0.3), 10, V, sampling=False) is None             # a warper: greedy / beams ignore it
    p = logits_processors(dict(min_new_tokens=4, suppress_tokens=[5, 1025], begin_suppress_tokens=[33],
                               exponential_decay_length_penalty=(6, 1.5), no_repeat_ngram_size=3, min_p=0.25), 17, V)
    assert (p.min_new_tokens, p.no_repeat_ngram_size, p.decay_start, p.prompt_len, p.n_suppress, p.n_begin_suppress) == (4, 3, 6, 17, 2, 1)
    assert abs(p.decay_factor - 1.5) < 1e-7 and abs(p.min_p - 0.25) < 1e-7
    assert p.suppress[0] == 1 << 5 and p.suppress[32] == 1 << 1 and p.begin_suppress[1] == 1 << 1
    for bad in (dict(min_new_tokens=-1), dict(min_length=2.5), dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=-2),
                dict(exponential_decay_length_penalty=(3, 0.0)), dict(exponential_decay_length_penalty=(3, -1.0)),
                dict(exponential_decay_length_penalty=3), dict(exponential_decay_length_penalty=(1.5, 2.0)),
                dict(suppress_tokens=[1026]), dict(begin_suppress_tokens=[-1]), dict(min_p=1.5), dict(min_p=-0.1)):
        with pytest.raises(ValueError):
            logits_processors(bad, 10, V)


def test_struct_layout_and_symbols():
    import ctypes as C
    from genvc_amd import _lib
    assert C.sizeof(_lib.LogitsProcessors) == 48 + 2 * 33 * 4
    assert _lib.LogitsProcessors.prompt_lens.offset == 40
    header = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    declared = set(re.findall(r"\b(gvc_[a-z0-9_]+)\s*\(", header))
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.exported_symbols(), s
    assert "#define GVC_PROC_MAX_NGRAM 8" in header


@pytest.mark.parametrize("flags", [["--min_new_tokens", "-3"], ["--no_repeat_ngram_size", "9"], ["--eos_decay", "4", "0"],
                                   ["--eos_decay", "4.5", "1.2"], ["--eos_decay", "4"], ["--min_p", "2"], ["--min_p", "x"]])
def test_infer_rejects_malformed_flags(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--synthetic", "--device", "cpu"] + flags, capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode != 0
    assert "bad processor flag" in r.stderr or "error:" in r.stderr or "must be" in r.stderr, r.stderr[-500:]
