"""CPU: speculative sampling for assisted decoding (GPT.generate(assistant_model=..., speculative_sampling=True)): the identity the rule
rests on in float64, the histogram of the CPU restatement (tests/spec_sample_oracle.py) against the target's distribution, the kwarg
table, the host loop through an engine stand-in, the CLI flag and the new C ABI."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_sample_oracle as SO               # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gvc_spec_accept_sample", "gvc_gpt_generate_assisted_sample")
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]
MODE = re.escape("assisted decoding (assistant_model)")


def cpu_gpt(max_slots=8, **more):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(**dict(dict(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"]), **more))
    g.max_slots = max_slots
    return g


def inputs(B=2, Tc=5):
    return torch.zeros(B, 32, D), torch.zeros(B, Tc, dtype=torch.long)


def ready(g):
    g.engine = type("E", (), dict(dims=g.dims()))()
    return g


# ---- 1. the identity ----------------------------------------------------------------------------------------------------------------
def test_accept_plus_residual_is_the_target_distribution():
    """q(y) min(1, p(y) / q(y)) + (1 - sum min(p, q)) resid(y) == p(y), resid = max(p - q, 0) normalised -- and p itself where p == q"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for case in range(200):
        V = int(rng.integers(2, 65))
        p, q = rng.random(V), rng.random(V)
        if case % 3 == 0:          # q with zeros where p > 0 (a draft that top-k'ed an id away), and p with zeros where q > 0
            q[rng.random(V) < 0.4] = 0.0
            p[rng.random(V) < 0.2] = 0.0
            q[0] = p[1] = 0.5
        p, q = p / p.sum(), q / q.sum()
        if case % 7 == 0:
            q = p.copy()
        acc = np.minimum(p, q)                       # q(y) min(1, p / q) without the division: q == 0 accepts, and is never drafted
        res = np.maximum(p - q, 0.0)
        rest = 1.0 - acc.sum()
        out = acc + (rest * res / res.sum() if res.sum() > 0 else rest * p)
        worst = max(worst, float(np.abs(out - p).max()))
    print(f"largest deviation {worst:.3e}")
    assert worst < 1e-12


# ---- 2. the restatement draws from the target's distribution --------------------------------------------------------------------------
@pytest.mark.parametrize("disjoint", [False, True], ids=["overlapping", "disjoint-top-k"])
def test_oracle_first_token_histogram(disjoint):
    """4096 first tokens (64 seeds x 64 rows, V = 32, position 1) against p_0 under the chi-square 0.999 quantile (Wilson-Hilferty);
    every expected count is at least 10, accepts and rejections both occur (never an accept with a disjoint draft), and the draws the
    1e-4 margins leave out are a small part (measured: 0.12 % / 0.27 %)"""
    case = SO.dist_case(disjoint)
    toks, low, acc = [], 0, 0
    for seed in SO.DIST_SEEDS:
        _, _, t, floor, a, p = SO.dist_round(case, seed)
        toks += list(t)
        low += int((floor <= 1e-4).sum())
        acc += int(a.sum())
    c, dof, emin, outside = SO.chi2(toks, p)
    bound = SO.chi2_bound(dof)
    print(f"chi2 {c:.1f} on {dof} degrees of freedom (bound {bound:.1f}), smallest expected count {emin:.1f}, accepted "
          f"{acc / len(toks):.3f}, below the margins {100.0 * low / len(toks):.2f} %")
    assert len(toks) == 4096 and dof == (14 if disjoint else 31) and abs(SO.chi2_bound(31) - 61.2) < 0.05
    assert emin >= 10.0 and outside == 0
    assert c < bound
    assert low <= 0.03 * len(toks)
    assert acc == 0 if disjoint else 0.2 * len(toks) < acc < 0.9 * len(toks)


def test_oracle_chain_accepts_its_own_drafts_and_keeps_the_budget():
    """the CPU chain (what whole generations are compared with on the GPU): a draft with the target's weights has q == p, so every
    draft is accepted and a row of 12 tokens takes 3 rounds (3 + 3 + 2 drafts behind the opening token); an unrelated draft changes the
    count of rounds, never the length or the range of the tokens"""
    from genvc_amd import synth
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    w = synth.make_weights(0, synth.gpt_weight_spec(dims))
    w["mel_head.bias"][1025] = -30.0
    other = synth.make_weights(5, synth.gpt_weight_spec(dims))
    cond, codes = synth.uniform(13, "cond_latents", (1, 32, dims["d_model"]), 1.0), synth.integers(13, "content_codes", (1, 6), 256)
    samp = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0)
    r = SO.generate(w, dims, w, dims, cond, codes, 3, samp, 1, 12)
    assert r["ids"].shape == (1, 12) and r["rounds"].tolist() == [3] and r["drafted"].tolist() == [8] and r["accepted"].tolist() == [8]
    u = SO.generate(w, dims, other, dims, cond, codes, 3, samp, 1, 12)
    assert u["ids"].shape == (1, 12) and u["rounds"][0] >= 3 and u["accepted"][0] <= u["drafted"][0] <= 3 * u["rounds"][0]
    assert u["ids"][0, 0] == r["ids"][0, 0]          # the opening token is the target's alone: u_res(0) on p_0
    assert int(u["ids"].max()) < 1026 and r["latents"].shape == (1, 12, dims["d_model"])


def test_position_keys_do_not_collide():
    """the three uniforms of a position and row are three different counters, and no (position, row) pair shares one with another"""
    seen = {}
    for b in range(8):
        for t in range(16):
            for name, f in (("draft", SO.u_draft), ("acc", SO.u_acc), ("res", SO.u_res)):
                seen.setdefault(f(5, t, b), []).append((name, t, b))
    assert all(len(v) == 1 for v in seen.values()) and len(seen) == 8 * 16 * 3
    assert SO.u_draft(5, 3, 1) == SO.O.rng_uniform(5, 3, 3) and SO.u_acc(5, 3, 1) == SO.O.rng_uniform(5, 3, 4)
    assert SO.u_res(5, 3, 1) == SO.O.rng_uniform(5, 3, 5)


# ---- 3. the kwarg table -------------------------------------------------------------------------------------------------------------
def test_accepted_combinations_reach_the_engine():
    g = cpu_gpt()
    cond, codes = inputs()
    for kw in (dict(), dict(do_sample=True, top_k=15, top_p=0.85, temperature=0.75, repetition_penalty=2.0, seed=3),
               dict(top_k=0, min_p=0.05, no_repeat_ngram_size=2, min_new_tokens=3), dict(do_sample=False), dict(top_k=1),
               dict(num_assistant_tokens=15, suppress_tokens=[3]), dict(typical_p=1.0)):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate(cond, codes, assistant_model=ready(cpu_gpt()), speculative_sampling=True, **kw)


def test_refused_combinations_raise_by_name():
    g = cpu_gpt(max_slots=16)
    cond, codes = inputs(B=1)
    a = ready(cpu_gpt())
    cases = [(dict(num_beams=4), r"beam search \(num_beams=4\) with " + MODE),
             (dict(num_beams=4, num_beam_groups=2, diversity_penalty=0.5), "beam groups .* with " + MODE),
             (dict(do_sample=False, top_k=4, penalty_alpha=0.6), r"contrastive search \(penalty_alpha=0.6\) with " + MODE),
             (dict(guidance_scale=2.0, negative_cond_latents=cond), r"guidance_scale=2.0 with " + MODE),
             (dict(num_return_sequences=3), "num_return_sequences=3 with " + MODE),
             (dict(return_dict_in_generate=True, output_scores=True), "output_scores=True with " + MODE),
             (dict(return_dict_in_generate=True, output_logits=True), "output_logits=True with " + MODE),
             (dict(sequence_bias={(5,): 1.0}), "sequence_bias=.* is not served with " + MODE),
             (dict(bad_words_ids=[[5]]), "bad_words_ids=.* is not served with " + MODE),
             (dict(forced_eos_token_id=1025), "forced_eos_token_id=.* is not served with " + MODE),
             (dict(renormalize_logits=True), "renormalize_logits=.* is not served with " + MODE),
             (dict(typical_p=0.9), "typical_p / epsilon_cutoff / eta_cutoff with " + MODE),
             (dict(epsilon_cutoff=0.01), "typical_p / epsilon_cutoff / eta_cutoff with " + MODE),
             (dict(eta_cutoff=0.01), "typical_p / epsilon_cutoff / eta_cutoff with " + MODE)]
    for kw, msg in cases:
        with pytest.raises(NotImplementedError, match=msg):
            g.generate(cond, codes, assistant_model=a, speculative_sampling=True, **kw)
    for sched in ("heuristic", "heuristic_transient"):
        with pytest.raises(ValueError, match=f"num_assistant_tokens_schedule='{sched}' with " + MODE):
            g.generate(cond, codes, assistant_model=a, speculative_sampling=True, num_assistant_tokens_schedule=sched)
    with pytest.raises(ValueError, match="speculative_sampling must be True, False or None"):
        g.generate(cond, codes, assistant_model=a, speculative_sampling="yes")


def test_without_the_kwarg_sampling_is_still_refused():
    g = cpu_gpt()
    cond, codes = inputs(B=1)
    a = ready(cpu_gpt())
    for kw in (dict(), dict(do_sample=True, top_k=15), dict(speculative_sampling=False), dict(speculative_sampling=None, top_k=15)):
        with pytest.raises(NotImplementedError, match=r"sampling \(do_sample=True, top_k=\d+\) with " + MODE + ".*speculative_sampling=True"):
            g.generate(cond, codes, assistant_model=a, **kw)


def test_other_paths_keep_refusing_an_assistant():
    g = cpu_gpt()
    cond, codes = inputs(B=1)
    kw = dict(assistant_model=ready(cpu_gpt()), speculative_sampling=True)
    for where, call in (("streaming (get_generator)", lambda: next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))),
                        ("grouped (generate_groups)", lambda: g.generate_groups([(cond, codes)], **kw)),
                        ("rolling (generate_rolling)", lambda: g.generate_rolling([(cond, codes)], **kw))):
        with pytest.raises(NotImplementedError, match=re.escape(f"assisted decoding (assistant_model) is not on the {where} path")):
            call()


# ---- 4. the host loop through a stand-in ------------------------------------------------------------------------------------------------
class StandIn:
    """an engine stand-in that plays the device's part of an assisted generation on the CPU: two tokens per round and row"""

    def __init__(self, g):
        self.dims = g.dims()
        self.calls = []

    def prefix_embeddings(self, cond, codes):
        return torch.zeros(cond.shape[0], cond.shape[1] + codes.shape[1] + 2, cond.shape[2])

    def prefill(self, slots, prefix, want_outputs=True, n_cached=0):
        self.calls.append(("prefill",))

    def generate_assisted(self, assistant, slots, aslots, st, params, n_rounds, max_keys, a_max_keys, proc=None, k=None, **more):
        self.calls.append(("generate_assisted", dict(more), params.top_k, round(params.top_p, 6), round(params.temperature, 6),
                           round(params.repetition_penalty, 6), params.seed, None if proc is None else round(proc.min_p, 6), k))
        for b in range(st.B):
            if not st.opened:
                st.toks[b, 0] = 7
                st.emitted[b] = 1
            for _ in range(n_rounds):
                if not st.finished[b]:
                    n = min(2, st.max_new - int(st.emitted[b]))
                    st.toks[b, int(st.emitted[b]):int(st.emitted[b]) + n] = 7
                    st.emitted[b] += n
                    st.rounds[b] += 1
                    st.finished[b] = int(st.emitted[b] >= st.max_new)
        st.opened = True

    def health(self):
        pass

    def reset(self, slots):
        pass


def test_host_loop_calls_the_engine_in_sampling_mode():
    g, a = cpu_gpt(), cpu_gpt()
    g.engine, a.engine = StandIn(g), StandIn(a)
    cond, codes = inputs(B=2)
    out = g.generate(cond, codes, assistant_model=a, speculative_sampling=True, top_k=15, top_p=0.85, temperature=0.75, seed=41,
                     repetition_penalty=2.0, min_p=0.05, num_assistant_tokens=3, max_new_tokens=9)
    assert out.shape == (2, 9) and bool((out == 7).all()) and g.last_latents.shape == (2, 9, D)
    assert set(g.last_assist_stats) == {"rounds", "drafted", "accepted"}
    calls = [c for c in g.engine.calls if c[0] == "generate_assisted"]
    assert calls and all(c[1:] == (dict(sampling=True), 15, 0.85, 0.75, 2.0, 41, 0.05, 3) for c in calls)
    # do_sample=False or top_k=1 with the kwarg, and any call without it: the greedy mode makes the call it made before (no `sampling`
    # argument, top_k 1, top_p 1, min_p a warper that greedy decoding does not build)
    for kw in (dict(speculative_sampling=True, do_sample=False, top_k=15, top_p=0.85), dict(speculative_sampling=True, top_k=1),
               dict(do_sample=False)):
        g.engine.calls.clear()
        g.generate(cond, codes, assistant_model=a, min_p=0.05, no_repeat_ngram_size=2, max_new_tokens=9, **kw)
        calls = [c for c in g.engine.calls if c[0] == "generate_assisted"]
        assert calls and all(c[1:4] == ({}, 1, 1.0) and c[7] == 0.0 for c in calls)
    with pytest.raises(ValueError, match="top_k=5000 is above the vocabulary"):
        g.generate(cond, codes, assistant_model=a, speculative_sampling=True, top_k=5000)
    with pytest.raises(ValueError, match="temperature=0.0 must be > 0"):
        g.generate(cond, codes, assistant_model=a, speculative_sampling=True, temperature=0.0)


def test_engine_entry_checks_its_arguments_on_the_host():
    """GptEngine.generate_assisted(sampling=True) asks the state for its sampling workspaces only then (none on a CPU-made state
    that is never asked), and engine.spec_accept_sample exists"""
    import genvc_amd.engine as E
    import inspect
    assert "sampling" in inspect.signature(E.GptEngine.generate_assisted).parameters
    assert inspect.signature(E.GptEngine.generate_assisted).parameters["sampling"].default is False
    assert callable(E.spec_accept_sample) and callable(E.AssistedState.sampling)
    st = E.AssistedState(torch.ones(2, 5, dtype=torch.int32), 3, 6, 1025, 1026, 8)
    assert getattr(st, "_sampling", None) is None
    ws = st.sampling()
    assert tuple(st.q_scores.shape) == tuple(st.p_scores.shape) == (2, 16, 1026) and st.key_rows.numel() == 2 * 32
    assert st.sampling() is ws and ws.q_scores == st.q_scores.data_ptr() and ws.rows == st.key_rows.data_ptr()


# ---- 5. CLI and C ABI -----------------------------------------------------------------------------------------------------------------
def _infer(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--device", "cpu", *flags], capture_output=True, text=True,
                          env=env, cwd=ROOT)


def test_infer_flag():
    r = _infer("--synthetic", "--assistant_sampling")
    assert r.returncode != 0 and "--assistant_sampling needs --assistant_layers" in r.stderr
    src = open(os.path.join(ROOT, "infer.py")).read()
    assert "speculative_sampling=True" in src and "--assistant_sampling" in open(os.path.join(ROOT, "README.md")).read()


def test_new_symbols_declared_and_exported():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    # the struct of the header, field for field, and the sizes the header's types give on LP64
    m = re.search(r"typedef struct gvc_spec_sampling \{(.*?)\} gvc_spec_sampling;", hdr, re.S)
    fields = re.findall(r"(\w+)\s*\*\s*(\w+);", m.group(1))
    assert [n for _, n in fields] == [n for n, _ in _lib.SpecSampling._fields_] == ["q_scores", "p_scores", "rows"]
    assert C.sizeof(_lib.SpecSampling) == 3 * C.sizeof(C.c_void_p) == 24
    assert C.sizeof(_lib.RowSampling) == 32 and _lib.RowSampling.seed.offset == 16          # what the round-begin kernel writes
    assert C.sizeof(_lib.SpecState) == 6 * 4 + 17 * 8
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s
