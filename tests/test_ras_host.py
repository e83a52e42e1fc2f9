"""CPU: repetition-aware sampling (ras_window / ras_threshold; include/genvc_hip.h: gvc_logits_ras) -- validation of the
kwargs and the integers the host hands the device, the refusals of the modes that do not serve it, by name, the per-item dicts, the
infer.py flags, the C ABI's struct, salt and symbols, and properties of the restatement tests/ras_oracle.py the GPU tests compare with."""
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

import ras_oracle as RO                    # noqa: E402
from genvc_amd import config as gcfg      # noqa: E402
from oracle import genvc_oracle as O      # noqa: E402

V, EOS = 1026, 1025
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]
SYMBOLS = ("gvc_sample_ras", "gvc_gpt_generate_ras")


def cpu_gpt(max_slots=16):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"])
    g.max_slots = max_slots
    return g


# ---- 1. the kwargs and the integers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,tau,want", [(10, 0.1, 1), (10, 0.3, 3), (1, 1.0, 1), (64, 0.1, 7), (7, 0.15, 2)])
def test_min_count_table(K, tau, want):
    from genvc_amd.engine import logits_ras, ras_counts
    assert ras_counts(dict(ras_window=K, ras_threshold=tau)) == (K, want)
    assert RO.min_count(K, tau) == want
    r = logits_ras(dict(ras_window=K, ras_threshold=tau), 41)
    assert (r.window, r.min_count, r.prompt_len, r.reserved) == (K, want, 41, 0)


def test_default_threshold_and_off_spellings():
    from genvc_amd.engine import RAS_KWARGS, logits_ras, ras_counts
    assert RAS_KWARGS == ("ras_window", "ras_threshold")
    assert ras_counts(dict(ras_window=10)) == (10, 1) and ras_counts(dict(ras_window=30)) == (30, 3)
    for off in ({}, dict(ras_window=None), dict(ras_window=0), dict(ras_window=None, ras_threshold=None)):
        assert ras_counts(off) is None and logits_ras(off, 40) is None


@pytest.mark.parametrize("bad", [dict(ras_window=65), dict(ras_window=-1), dict(ras_window=2.5), dict(ras_window=10.0), dict(ras_window="8"),
                                 dict(ras_window=True), dict(ras_window=False), dict(ras_window=10, ras_threshold=0.0),
                                 dict(ras_window=10, ras_threshold=1.5), dict(ras_window=10, ras_threshold=-0.1),
                                 dict(ras_window=10, ras_threshold="x"), dict(ras_window=10, ras_threshold=True),
                                 dict(ras_window=10, ras_threshold=float("nan")), dict(ras_threshold=0.2),
                                 dict(ras_window=0, ras_threshold=0.2)])
def test_argument_errors_are_value_errors(bad):
    from genvc_amd.engine import ras_counts
    with pytest.raises(ValueError, match="ras_window|ras_threshold"):
        ras_counts(bad)
    g = cpu_gpt()
    with pytest.raises(ValueError, match="ras_window|ras_threshold"):
        g.generate(torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long), top_k=15, **bad)
    with pytest.raises(ValueError, match="ras_window|ras_threshold"):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), top_k=15, **bad))


def test_threshold_without_window_names_both():
    from genvc_amd.engine import ras_counts
    with pytest.raises(ValueError, match="ras_threshold=0.2 without ras_window"):
        ras_counts(dict(ras_threshold=0.2))


# ---- 2. refusals, by name ---------------------------------------------------------------------------------------------------------
def test_modes_refuse_by_name():
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    named = re.escape("ras_window=10 with ")
    with pytest.raises(NotImplementedError, match=named + re.escape("beam search (num_beams=4)")):
        g.generate(cond, codes, num_beams=4, do_sample=False, ras_window=10)
    with pytest.raises(NotImplementedError, match=named + "beam groups"):
        g.generate(cond, codes, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, do_sample=False, ras_window=10)
    with pytest.raises(NotImplementedError, match=named + re.escape("contrastive search (penalty_alpha=0.6)")):
        g.generate(cond, codes, do_sample=False, top_k=4, penalty_alpha=0.6, ras_window=10)
    for extra in (dict(do_sample=False), dict(top_k=1), dict(speculative_sampling=True, top_k=15)):          # greedy and speculative
        with pytest.raises(NotImplementedError, match=named + re.escape("assisted decoding (assistant_model)")):
            g.generate(cond, codes, assistant_model=cpu_gpt(), ras_window=10, **extra)
        with pytest.raises(NotImplementedError, match=named + re.escape("prompt-lookup decoding (prompt_lookup_num_tokens)")):
            g.generate(cond, codes, prompt_lookup_num_tokens=4, ras_window=10, **extra)
    with pytest.raises(NotImplementedError, match=named + "beam search"):
        g.generate(cond, codes, num_beams=2, do_sample=False, guidance_scale=1.5, negative_cond_latents=cond, ras_window=10)


def test_greedy_search_points_to_top_k_1():
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    with pytest.raises(ValueError, match=r"ras_window=10 with do_sample=False.*do_sample=True with top_k=1"):
        g.generate(cond, codes, do_sample=False, ras_window=10)
    with pytest.raises(ValueError, match=r"do_sample=True with top_k=1"):
        g.generate_groups([(cond, codes)], do_sample=False, ras_window=10)
    with pytest.raises(ValueError, match=r"do_sample=True with top_k=1"):
        g.generate_rolling([(cond, codes)], do_sample=False, ras_window=10)
    # off spellings and a served call reach the engine check as ever
    for kw in (dict(ras_window=None), dict(ras_window=0), dict(ras_window=10, top_k=1), dict(ras_window=10, ras_threshold=0.3)):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate(cond, codes, **kw)


# ---- 3. per-item dicts ------------------------------------------------------------------------------------------------------------
def test_per_item_dicts_carry_ras_with_the_sets():
    from genvc_amd.engine import ProcessorSets, WarperSets, check_proc_kwargs, logits_sets
    from genvc_amd.layers.gpt import _per_item_procs
    from genvc_amd.streaming import StreamSessions
    check_proc_kwargs(dict(ras_window=10, ras_threshold=0.2, min_p=0.1), "row 0")
    kws = [dict(ras_window=10), None, dict(ras_window=10, min_new_tokens=3), dict(ras_window=10), dict(typical_p=0.5), dict(ras_window=0)]
    ws = logits_sets(kws, [40, 40, 40, 41, 40, 40], V)
    assert isinstance(ws, WarperSets) and ws.ras is not None
    assert list(ws.set_of_row) == [0, -1, 1, 2, 3, -1]          # (rows 0 and 3 count from different prompts: entries of their own)
    assert ws.n_sets == 4 and ws.ras.n == 4
    assert [(r.window, r.min_count, r.prompt_len) for r in ws.ras.ras] == [(10, 1, 40), (10, 1, 40), (10, 1, 41), (0, 0, 0)]
    assert ws.sets[1].min_new_tokens == 3 and ws.warps[3].typical_p == pytest.approx(0.5)
    # no RAS anywhere: exactly what the call returned before
    plain = logits_sets([dict(min_new_tokens=3), None, dict(ras_window=None)], 40, V)
    assert isinstance(plain, ProcessorSets) and not hasattr(plain, "ras")
    assert logits_sets([dict(typical_p=0.5), None], 40, V).ras is None
    with pytest.raises(ValueError, match=r"row 1: ras_window"):
        logits_sets([None, dict(ras_window=70)], 40, V)
    with pytest.raises(ValueError, match=re.escape("group_kwargs[0]: ras_window")):
        _per_item_procs({}, [dict(ras_window=-2)], 1, "group_kwargs", V)
    merged = _per_item_procs(dict(ras_window=8, ras_threshold=0.5), [None, dict(ras_window=0, ras_threshold=None)], 2, "job_kwargs", V)
    assert merged[0] == dict(ras_window=8, ras_threshold=0.5) and merged[1]["ras_window"] == 0
    with pytest.raises(ValueError, match=r"open: ras_threshold"):
        StreamSessions._procs(type("S", (), {"m": type("M", (), {"gpt": type("G", (), {"num_audio_tokens": V})()})()})(),
                              dict(ras_window=10, ras_threshold=2.0), {}, "open")


# ---- 4. the command line ----------------------------------------------------------------------------------------------------------
def _infer(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--device", "cpu", *flags], capture_output=True, text=True,
                          env=env, cwd=ROOT, timeout=120)


def test_infer_flags():
    r = _infer("--help")
    assert r.returncode == 0 and "--ras_window" in r.stdout and "--ras_threshold" in r.stdout
    # good values pass the RAS checks, with and without --streaming: the run ends at a later check of another flag
    for flags in (("--ras_window", "10"), ("--ras_window", "10", "--ras_threshold", "0.3", "--streaming"), ("--ras_window", "64", "--top_k", "1")):
        r = _infer(*flags, "--min_p", "2")
        assert r.returncode != 0 and "bad processor flag: min_p" in r.stderr, r.stderr[-400:]
    for flags, msg in ((("--ras_window", "65"), "--ras_window must be in 0..64"), (("--ras_window", "-1"), "--ras_window must be in 0..64"),
                       (("--ras_window", "10", "--ras_threshold", "0"), "--ras_threshold in (0, 1]"),
                       (("--ras_window", "10", "--ras_threshold", "1.5"), "--ras_threshold in (0, 1]"),
                       (("--ras_threshold", "0.2"), "--ras_threshold needs --ras_window"),
                       (("--ras_window", "x"), "invalid int value"), (("--ras_window", "2.5"), "invalid int value"),
                       (("--ras_window", "10", "--num_beams", "4"), "--ras_window does not combine with --num_beams"),
                       (("--ras_window", "10", "--penalty_alpha", "0.6", "--top_k", "4"), "--ras_window does not combine"),
                       (("--ras_window", "10", "--prompt_lookup_num_tokens", "4"), "--ras_window does not combine")):
        r = _infer(*flags)
        assert r.returncode != 0 and msg in r.stderr, (flags, r.stderr[-400:])


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------
def test_struct_salt_and_symbols():
    from genvc_amd import _lib
    assert C.sizeof(_lib.LogitsRas) == 16
    assert [f for f, _ in _lib.LogitsRas._fields_] == ["window", "min_count", "prompt_len", "reserved"]
    assert _lib.RAS_SALT == RO.SALT == 0x5241535F52454452 == int.from_bytes(b"RAS_REDR", "big")
    header = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    assert re.search(r"typedef struct gvc_logits_ras \{\s*int32_t window;[^}]*int32_t min_count;[^}]*int32_t prompt_len;[^}]*int32_t reserved;"
                     r"[^}]*\} gvc_logits_ras;", header)
    assert re.search(r"#define GVC_RAS_SALT 0x5241535F52454452ull", header) and re.search(r"#define GVC_RAS_MAX_WINDOW 64\b", header)
    declared = set(re.findall(r"\b(gvc_[a-z0-9_]+)\s*\(", header))
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib.exported_symbols(), s
    body = open(os.path.join(ROOT, "genvc_amd", "csrc", "sample_body.h")).read()
    assert "GVC_RAS_SALT" in body


# ---- 6. the restatement -----------------------------------------------------------------------------------------------------------
SAMP = dict(repetition_penalty=1.0, temperature=0.85, top_p=0.85, top_k=15)


def _logits(seed):
    return torch.randn(V, generator=torch.Generator().manual_seed(seed)) * 2.0


def test_unreachable_count_is_the_plain_sampler():
    """min_count > K can only be set by hand; no window can hold that many, so every step is the plain sampler's step, which is
    oracle.genvc_oracle's process_logits + sample_from_scores"""
    rng = np.random.default_rng(3)
    for seed in range(12):
        lg = _logits(seed)
        row = [int(t) for t in rng.integers(0, 1024, size=30)]
        r = RO.step(lg, row, 6, SAMP, {}, (10, 11), (seed, 5, 0), EOS)
        scores = O.process_logits(lg[None], torch.tensor([row]), 1.0, 0.85, 15, 0.85)
        assert not r["redraw"] and r["tok"] == r["x"] == int(O.sample_from_scores(scores, seed, 5)[0])
        assert r == RO.step(lg, row, 6, SAMP, {}, None, (seed, 5, 0), EOS)


def test_single_survivor_redraws_from_min_count_on():
    """a row whose truncated set is one token (top_k = 1) emits it until the window holds min_count of them, and from n_gen >= min_count
    on every step redraws"""
    lg = _logits(40)
    x = int(torch.argmax(lg))
    samp = dict(SAMP, top_k=1)
    for K, mc in ((10, 1), (10, 3), (4, 4)):
        row = [1] * 6
        for step in range(12):
            r = RO.step(lg, row, 6, samp, {}, (K, mc), (9, step, 0), EOS)
            assert r["x"] == x and r["c"] == min(step, K) and r["redraw"] == (step >= mc)
            row.append(x)          # (teacher-forced: the history keeps repeating whatever the redraw gave)


def test_prompt_ids_never_count_and_window_edges():
    lg = _logits(41)
    x = int(torch.argmax(lg))
    samp = dict(SAMP, top_k=1)
    assert not RO.step(lg, [x] * 6, 6, samp, {}, (10, 1), (1, 0, 0), EOS)["redraw"]                    # n_gen = 0
    assert not RO.step(lg, [x] * 6 + [2, 3], 6, samp, {}, (10, 1), (1, 0, 0), EOS)["redraw"]           # only in the prompt
    row = [1] * 6 + [x] + [2] * 10
    assert not RO.step(lg, row, 6, samp, {}, (10, 1), (1, 0, 0), EOS)["redraw"]                        # at len - K - 1
    assert RO.step(lg, row[:-1], 6, samp, {}, (10, 1), (1, 0, 0), EOS)["redraw"]                       # at len - K
    fin = RO.step(lg, row[:-1], 6, samp, {}, (10, 1), (1, 0, 0), EOS, finished=True)
    assert not fin["redraw"] and fin["tok"] == EOS


def test_redraw_uses_the_salted_key_and_the_full_row():
    lg = _logits(42)
    samp = dict(SAMP, top_k=1)
    x = int(torch.argmax(lg))
    row = [1] * 6 + [x]
    kw = dict(suppress_tokens=[5, 6, 7])
    got = RO.step(lg, row, 6, samp, kw, (1, 1), (77, 3, 2), EOS)
    full = RO.full_row(lg, row, 6, samp, kw, EOS)
    assert got["redraw"] and got["tok"] == RO.draw(full, O.rng_uniform(77 ^ RO.SALT, 3, 2))[0]
    assert all(full[t] == -float("inf") for t in (5, 6, 7)) and int(torch.isfinite(full).sum()) == V - 3
    toks = {RO.step(lg, row, 6, samp, kw, (1, 1), (s, 3, 2), EOS)["tok"] for s in range(200)}
    assert len(toks) > 20 and not toks & {5, 6, 7}
