"""CPU: the presence / frequency / windowed repetition penalties (presence_penalty / frequency_penalty / penalty_window;
include/genvc_hip.h: gvc_logits_penalties) -- validation of the kwargs, the off spellings that pass no table, the
refusals of the modes that do not serve them, by name, the per-item dicts, the infer.py flags, the C ABI's struct and symbols, and the
restatement tests/penalty_oracle.py the GPU tests compare with, checked against transformers and an independent float64 computation."""
import ctypes as C
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

import penalty_oracle as PN                # noqa: E402
from genvc_amd import config as gcfg      # noqa: E402

V, EOS = 1026, 1025
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]
SYMBOLS = ("gvc_sample_pen", "gvc_gpt_generate_pen")


def cpu_gpt(max_slots=16):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"])
    g.max_slots = max_slots
    return g


# ---- 1. the kwargs ----------------------------------------------------------------------------------------------------------------
def test_kwargs_and_struct_values():
    from genvc_amd.engine import PENALTY_KWARGS, logits_penalties, penalty_settings
    assert PENALTY_KWARGS == ("presence_penalty", "frequency_penalty", "penalty_window")
    assert penalty_settings(dict(presence_penalty=0.5)) == (0.5, 0.0, 0)
    assert penalty_settings(dict(frequency_penalty=-2, penalty_window=16)) == (0.0, -2.0, 16)
    assert penalty_settings(dict(penalty_window=16, repetition_penalty=2.0)) == (0.0, 0.0, 16)          # the windowed repetition penalty alone
    q = logits_penalties(dict(presence_penalty=0.25, frequency_penalty=1.5, penalty_window=7), 41)
    assert (q.presence, q.frequency, q.window, q.prompt_len) == (0.25, 1.5, 7, 41)


@pytest.mark.parametrize("off", [{}, dict(presence_penalty=None), dict(presence_penalty=0), dict(frequency_penalty=0.0),
                                 dict(presence_penalty=0.0, frequency_penalty=None, penalty_window=0), dict(penalty_window=None),
                                 dict(presence_penalty=-0.0, frequency_penalty=0, penalty_window=None)])
def test_off_spellings_pass_no_table(off):
    from genvc_amd.engine import ProcessorSets, logits_penalties, logits_sets, penalty_settings
    assert penalty_settings(off) is None and logits_penalties(off, 40) is None
    assert logits_sets([off, None], 40, V) is None
    plain = logits_sets([dict(off, min_new_tokens=3), None], 40, V)
    assert isinstance(plain, ProcessorSets) and not hasattr(plain, "pen")
    # the loop state of a call carries no table, and generate_call then takes the entry it took before
    from genvc_amd.engine import GptEngine
    calls = []

    class Eng:
        def generate(self, *a, **k):
            calls.append("generate")

        def generate_pen(self, *a, **k):
            calls.append("generate_pen")
    slots = torch.zeros(2, dtype=torch.int32)
    GptEngine.generate_call(Eng(), slots, None, None, None, None, 0, 1, None, None, pen=None)
    assert calls == ["generate"]


@pytest.mark.parametrize("bad", [dict(presence_penalty=2.5), dict(presence_penalty=-2.01), dict(frequency_penalty=3), dict(frequency_penalty=-5.0),
                                 dict(presence_penalty=float("nan")), dict(frequency_penalty=float("inf")), dict(presence_penalty=-float("inf")),
                                 dict(presence_penalty=True), dict(frequency_penalty=False), dict(presence_penalty="0.5"),
                                 dict(penalty_window=-1), dict(penalty_window=2.5), dict(penalty_window=8.0), dict(penalty_window="8"),
                                 dict(penalty_window=True), dict(penalty_window=False), dict(presence_penalty=0.5, penalty_window=-3)])
def test_argument_errors_are_value_errors(bad):
    from genvc_amd.engine import penalty_settings
    named = "presence_penalty|frequency_penalty|penalty_window"
    with pytest.raises(ValueError, match=named):
        penalty_settings(bad)
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    with pytest.raises(ValueError, match=named):
        g.generate(cond, codes, top_k=15, **bad)
    with pytest.raises(ValueError, match=named):
        g.generate(cond, codes, do_sample=False, **bad)
    with pytest.raises(ValueError, match=named):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), top_k=15, **bad))
    with pytest.raises(ValueError, match=named):
        g.generate_groups([(cond, codes)], **bad)
    with pytest.raises(ValueError, match=named):
        g.generate_rolling([(cond, codes)], top_k=1, **bad)


def test_range_edges_are_served():
    from genvc_amd.engine import penalty_settings
    assert penalty_settings(dict(presence_penalty=2, frequency_penalty=-2.0)) == (2.0, -2.0, 0)
    assert penalty_settings(dict(penalty_window=100000)) == (0.0, 0.0, 100000)


# ---- 2. refusals, by name ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pkw,named", [(dict(presence_penalty=0.5), "presence_penalty=0.5 with "),
                                       (dict(frequency_penalty=0.25), "frequency_penalty=0.25 with "),
                                       (dict(penalty_window=16, repetition_penalty=2.0), "penalty_window=16 with ")])
def test_modes_refuse_by_name(pkw, named):
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    named = re.escape(named)
    with pytest.raises(NotImplementedError, match=named + re.escape("beam search (num_beams=4)")):
        g.generate(cond, codes, num_beams=4, do_sample=False, **pkw)
    with pytest.raises(NotImplementedError, match=named + "beam groups"):
        g.generate(cond, codes, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, do_sample=False, **pkw)
    with pytest.raises(NotImplementedError, match=named + re.escape("contrastive search (penalty_alpha=0.6)")):
        g.generate(cond, codes, do_sample=False, top_k=4, penalty_alpha=0.6, **pkw)
    for extra in (dict(do_sample=False), dict(top_k=1), dict(speculative_sampling=True, top_k=15)):
        with pytest.raises(NotImplementedError, match=named + re.escape("assisted decoding (assistant_model)")):
            g.generate(cond, codes, assistant_model=cpu_gpt(), **pkw, **extra)
        with pytest.raises(NotImplementedError, match=named + re.escape("prompt-lookup decoding (prompt_lookup_num_tokens)")):
            g.generate(cond, codes, prompt_lookup_num_tokens=4, **pkw, **extra)


def test_greedy_and_served_calls_reach_the_engine_check():
    """do_sample=False is fine (greedy decoding uses the penalties too), as are the off spellings: the call ends where every call on a
    GPT without an engine ends"""
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    for kw in (dict(presence_penalty=0.5, do_sample=False), dict(frequency_penalty=0.5, top_k=1), dict(presence_penalty=None),
               dict(penalty_window=0), dict(penalty_window=16, repetition_penalty=2.0), dict(presence_penalty=0.5, ras_window=4),
               dict(frequency_penalty=0.5, guidance_scale=1.5, negative_cond_latents=cond), dict(presence_penalty=1.0, num_return_sequences=2)):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate(cond, codes, **kw)


# ---- 3. per-item dicts ------------------------------------------------------------------------------------------------------------
def test_per_item_dicts_carry_penalties_with_the_sets():
    from genvc_amd.engine import WarperSets, check_proc_kwargs, logits_sets
    from genvc_amd.layers.gpt import _per_item_procs
    from genvc_amd.streaming import StreamSessions
    check_proc_kwargs(dict(presence_penalty=0.5, frequency_penalty=0.1, penalty_window=8, min_p=0.1, ras_window=4), "row 0")
    with pytest.raises(ValueError, match="'penalty_windows' is not a processor kwarg"):
        check_proc_kwargs(dict(penalty_windows=8), "row 0")
    kws = [dict(presence_penalty=0.5), None, dict(presence_penalty=0.5, min_new_tokens=3), dict(presence_penalty=0.5),
           dict(typical_p=0.5), dict(frequency_penalty=0), dict(penalty_window=8, ras_window=4)]
    ws = logits_sets(kws, [40, 40, 40, 41, 40, 40, 40], V)
    assert isinstance(ws, WarperSets) and ws.pen is not None and ws.ras is not None
    assert list(ws.set_of_row) == [0, -1, 1, 2, 3, -1, 4]          # (rows 0 and 3 count from different prompts: entries of their own)
    assert ws.n_sets == 5 and ws.pen.n == 5 and ws.ras.n == 5
    assert [(q.presence, q.frequency, q.window, q.prompt_len) for q in ws.pen.pen] == [(0.5, 0.0, 0, 40), (0.5, 0.0, 0, 40), (0.5, 0.0, 0, 41),
                                                                                    (0.0, 0.0, 0, 0), (0.0, 0.0, 8, 40)]
    assert logits_sets([dict(typical_p=0.5), None], 40, V).pen is None
    with pytest.raises(ValueError, match=r"row 1: presence_penalty"):
        logits_sets([None, dict(presence_penalty=7)], 40, V)
    with pytest.raises(ValueError, match="host prompt length"):
        logits_sets([dict(presence_penalty=0.5)], 40, V, prompt_lens=torch.tensor([40], dtype=torch.int32))
    with pytest.raises(ValueError, match=re.escape("group_kwargs[0]: penalty_window")):
        _per_item_procs({}, [dict(penalty_window=-2)], 1, "group_kwargs", V)
    merged = _per_item_procs(dict(presence_penalty=0.5, penalty_window=8), [None, dict(presence_penalty=0, penalty_window=None)], 2,
                             "job_kwargs", V)
    assert merged[0] == dict(presence_penalty=0.5, penalty_window=8) and merged[1]["presence_penalty"] == 0
    sess = type("S", (), {"m": type("M", (), {"gpt": type("G", (), {"num_audio_tokens": V})()})()})()
    assert StreamSessions._procs(sess, dict(frequency_penalty=0.3), {}, "open") == dict(frequency_penalty=0.3)
    with pytest.raises(ValueError, match=r"open: frequency_penalty"):
        StreamSessions._procs(sess, dict(frequency_penalty=2.5), {}, "open")


def test_engine_refuses_a_table_that_does_not_fit_its_sets():
    from genvc_amd.engine import GptEngine, PenaltyTable, WarperSets, logits_penalties
    q = logits_penalties(dict(presence_penalty=0.5), 40)
    with pytest.raises(ValueError, match="2 penalty entries for 1 sets"):
        GptEngine._pen_args(None, PenaltyTable([q, q]), None)
    assert len(GptEngine._pen_args(None, PenaltyTable([q]), WarperSets([None], [None], [0, 0]))) == 1


# ---- 4. the command line ----------------------------------------------------------------------------------------------------------
def _infer(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--device", "cpu", *flags], capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=120)


def test_infer_flags():
    r = _infer("--help")
    assert r.returncode == 0 and all(f in r.stdout for f in ("--presence_penalty", "--frequency_penalty", "--penalty_window"))
    # good values pass the checks, with and without --streaming: the run ends at a later check of another flag
    for flags in (("--presence_penalty", "0.5"), ("--frequency_penalty", "-0.3", "--penalty_window", "16", "--streaming"),
                  ("--penalty_window", "16", "--top_k", "1")):
        r = _infer(*flags, "--min_p", "2")
        assert r.returncode != 0 and "bad processor flag: min_p" in r.stderr, r.stderr[-400:]
    for flags, msg in ((("--presence_penalty", "2.5"), "--presence_penalty must be in [-2, 2]"),
                       (("--frequency_penalty", "-3"), "--frequency_penalty must be in [-2, 2]"),
                       (("--frequency_penalty", "nan"), "--frequency_penalty must be in [-2, 2]"),
                       (("--penalty_window", "-1"), "--penalty_window must be >= 0"),
                       (("--penalty_window", "2.5"), "invalid int value"),
                       (("--presence_penalty", "0.5", "--num_beams", "4"), "do not combine with --num_beams"),
                       (("--penalty_window", "8", "--prompt_lookup_num_tokens", "4"), "do not combine")):
        r = _infer(*flags)
        assert r.returncode != 0 and msg in r.stderr, (flags, r.stderr[-400:])


# ---- 5. the C ABI -----------------------------------------------------------------------------------------------------------------
def test_struct_and_symbols():
    from genvc_amd import _lib
    assert C.sizeof(_lib.LogitsPenalties) == 16
    assert [(f, t) for f, t in _lib.LogitsPenalties._fields_] == [("presence", C.c_float), ("frequency", C.c_float), ("window", C.c_int32),
                                                                  ("prompt_len", C.c_int32)]
    header = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    assert re.search(r"typedef struct gvc_logits_penalties \{\s*float presence;[^}]*float frequency;[^}]*int32_t window;[^}]*"
                     r"int32_t prompt_len;[^}]*\} gvc_logits_penalties;", header)
    declared = set(re.findall(r"\b(gvc_[a-z0-9_]+)\s*\(", header))
    with open(_lib.LIB_PATH, "rb") as f:          # the built library: its dynamic string table names what it exports
        built = f.read()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib._SIGNATURES, s
        assert s in _lib.exported_symbols(), s
        assert s.encode() + b"\0" in built, f"{s} is not in {_lib.LIB_PATH}"


# ---- 6. the restatement -----------------------------------------------------------------------------------------------------------
def _logits(seed):
    return torch.randn(V, generator=torch.Generator().manual_seed(seed)) * 2.0


def _history(seed, plen, n_gen):
    rng = np.random.default_rng(seed)
    return [int(t) for t in rng.integers(0, 40, size=plen)] + [int(t) for t in rng.integers(30, 90, size=n_gen)]


@pytest.mark.parametrize("W,n_gen", [(1, 12), (5, 12), (12, 12), (40, 12), (8, 0), (3, 1)])
@pytest.mark.parametrize("rep", [1.3, 2.0, 0.7])
def test_windowed_repetition_penalty_is_transformers_on_the_window(W, n_gen, rep):
    """penalty_window = W with f = p = 0: the oracle's row is transformers' RepetitionPenaltyLogitsProcessor(rep) applied with
    input_ids = the last min(W, n_gen) generated ids"""
    from transformers import RepetitionPenaltyLogitsProcessor
    plen = 6
    for seed in range(4):
        lg = _logits(seed)
        row = _history(100 + seed, plen, n_gen)
        got = PN.penalised(lg, row, plen, rep, (0.0, 0.0, W))
        w = min(W, n_gen)
        tail = row[len(row) - w:] if w else []
        want = lg.clone()[None]
        if tail:
            want = RepetitionPenaltyLogitsProcessor(rep)(torch.tensor([tail], dtype=torch.long), want)
        assert torch.equal(got, want[0]), (seed, W, n_gen)
        if w < n_gen or any(t not in tail for t in row[:plen]):
            # without the window the repetition penalty covers the whole row, the fake prompt included
            assert not torch.equal(got, PN.penalised(lg, row, plen, rep, None))


@pytest.mark.parametrize("p,f,W", [(0.5, 0.0, 0), (0.0, 0.3, 0), (0.7, 0.11, 5), (-0.4, -0.2, 0), (1.3, 0.013, 300), (2.0, 2.0, 1)])
def test_frequency_and_presence_match_an_independent_float64_computation(p, f, W):
    """rep = 1: the oracle's row is the raw row minus f * bincount + p * (bincount > 0), computed in float64 and rounded to fp32
    operation by operation in the fixed order"""
    plen = 6
    for seed, n_gen in ((0, 0), (1, 1), (2, 30), (3, 400)):
        lg = _logits(seed)
        row = _history(200 + seed, plen, n_gen) + ([-1, V + 3] if seed == 2 else [])          # (ids outside the vocabulary are ignored)
        got = PN.penalised(lg, row, plen, 1.0, (p, f, W))
        gen = row[plen:]
        tail = gen[len(gen) - min(W, len(gen)):] if W else gen
        c = np.zeros(V, dtype=np.int64)
        for t in tail:
            if 0 <= t < V:
                c[t] += 1
        f32 = np.float32
        t1 = (np.float64(f32(f)) * c.astype(np.float64)).astype(f32)
        t2 = (t1.astype(np.float64) + np.float64(f32(p))).astype(f32)
        want = lg.numpy().copy()
        on = c > 0
        want[on] = (lg.numpy().astype(np.float64)[on] - t2.astype(np.float64)[on]).astype(f32)
        assert np.array_equal(got.numpy(), want), (seed, p, f, W)
        assert np.array_equal(PN.counts(row, plen, W, V).numpy(), c)
        if n_gen and not W:
            assert int(c.sum()) == n_gen


def test_counts_forget_the_prompt_and_ignore_ids_outside_the_vocabulary():
    row = [7, 7, 7] + [7, -1, 5000, 9, 7]
    assert PN.counts(row, 3, 0, V)[7] == 2 and PN.counts(row, 3, 0, V)[9] == 1 and int(PN.counts(row, 3, 0, V).sum()) == 3
    assert PN.counts(row, 3, 1, V)[7] == 1 and PN.counts(row, 3, 2, V)[9] == 1 and PN.counts(row, 3, 2, V)[7] == 1
    assert PN.counts(row, 3, 4, V)[7] == 1 and PN.counts(row, 3, 5, V)[7] == 2 and PN.counts(row, 3, 50, V)[7] == 2
    assert int(PN.counts(row[:3], 3, 0, V).sum()) == 0


def test_off_settings_are_the_plain_oracle_and_the_chain_order():
    """every off spelling is ras_oracle's row; the penalties sit ahead of the processors (a suppressed id stays -inf) and of Temperature"""
    import ras_oracle as RO
    samp = dict(repetition_penalty=1.3, temperature=0.8, top_p=0.85, top_k=15)
    lg = _logits(9)
    row = _history(9, 6, 20)
    kw = dict(suppress_tokens=[row[-1]], min_new_tokens=50)
    for off in (None, (0.0, 0.0, 0)):
        assert torch.equal(PN.full_row(lg, row, 6, samp, kw, EOS, off), RO.full_row(lg, row, 6, samp, kw, EOS))
        assert PN.step(lg, row, 6, samp, kw, off, (3, 5, 1), EOS) == RO.step(lg, row, 6, samp, kw, None, (3, 5, 1), EOS)
    on = PN.full_row(lg, row, 6, samp, kw, EOS, (0.5, 0.25, 0))
    assert on[row[-1]] == -float("inf") and on[EOS] == -float("inf")
    x = row[-2]
    c = int(PN.counts(row, 6, 0, V)[x])
    base = PN.penalised(lg, row, 6, 1.3, None)[x]
    t = torch.tensor(0.25) * torch.tensor(float(c)) + torch.tensor(0.5)
    assert on[x] == (base - t) / torch.tensor(0.8)
