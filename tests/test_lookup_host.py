"""CPU: prompt-lookup assisted decoding (GPT.generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=N)): the rule's numpy
restatement on crafted histories (and against transformers' PromptLookupCandidateGenerator where that imports), the greedy chain on
the oracle against plain greedy, the sampled chain's one-hot rule against tests/spec_sample_oracle.py's rule on explicit one-hot rows,
the accept restatements with a draft count per row, the validation of the kwargs and the paths that refuse them by name, the host loop
through an engine stand-in, infer.py's flags, and the new C ABI symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assist_oracle as AO                    # noqa: E402
import lookup_oracle as LO                    # noqa: E402
import spec_sample_oracle as SO               # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gvc_spec_lookup", "gvc_spec_accept_len", "gvc_spec_accept_sample_len", "gvc_gpt_generate_lookup")
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]
MODE = re.escape("prompt-lookup decoding (prompt_lookup_num_tokens)")
EOS, V = 1025, 1026
KEEP = (7, 300, 1000)                         # the codes a generation may use: n-grams must recur
SUPPRESS = [i for i in range(V) if i not in KEEP + (EOS,)]


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_rule_on_crafted_histories():
    L = LO.lookup
    assert L([], 3, 2) == [] and L([5], 3, 2) == []                           # nothing to look behind
    assert L([5, 5], 3, 2) == [5]                                             # n = 1: h[0] == suffix, one id behind it
    assert L([1, 2, 3, 4], 3, 2) == []                                        # only the suffix itself matches
    assert L([1, 2, 9, 8, 1, 2, 7, 6, 1, 2], 3, 2) == [9, 8, 1]               # two matches: the earliest wins
    assert L([2, 5, 5, 1, 2, 6, 6, 1, 2], 2, 2) == [6, 6]                     # n = 2 at index 3 beats n = 1 at index 0
    assert L([2, 5, 5, 1, 2, 6, 6, 1, 2], 2, 1) == [5, 5]                     # ... which N = 1 finds
    assert L([4, 1, 2, 3, 1, 2], 5, 2) == [3, 1, 2]                           # the continuation is cut at the end
    assert L([1, 2, 1, 2, 1, 2], 4, 2) == [1, 2, 1, 2]                        # periodic: the drafts overlap the suffix
    assert L([3, 3, 3], 15, 8) == [3]                                         # n = 2: [3, 3] at 0, one id behind it
    assert L([1, 2, 3, 1, 2, 3], 15, 8) == [1, 2, 3]                          # min(N, len - 1) = 5 down to 3


def test_rows_restatement_fills_what_the_kernel_fills():
    ids = np.array([[9, 9, 1, 2, 1, 0, 0], [9, 9, 4, 4, 4, 4, 0], [9, 9, 1, 2, 1, 2, 1]], dtype=np.int32)
    v, dl, q = LO.lookup_rows(ids, np.array([5, 6, 7]), np.array([0, 1, 0]), np.array([1, 4, 1]), 3, 2, 2, vocab=8)
    assert v.tolist() == [[1, 2, 1, 1], [4, 4, 4, 4], [1, 2, 1, 1]] and dl.tolist() == [2, 0, 2]
    assert np.isnan(q[:, 0]).all() and np.isnan(q[1]).all()
    for b in (0, 2):
        for j in (1, 2, 3):          # (column 3 is the filler: its row is one-hot at the pending token)
            w, _ = SO.weights(torch.from_numpy(q[b, j]))
            p = w / w.sum()
            assert p[v[b, j]] == 1.0 and p.sum() == 1.0                       # one-hot, as probabilities, exactly
    # the placeholders before `start` equal the suffix and do not match
    v, dl, _ = LO.lookup_rows(np.array([[1, 2, 7, 7, 1, 2]], dtype=np.int32), np.array([6]), np.array([0]), np.array([2]), 3, 2, 2)
    assert dl.tolist() == [0] and v.tolist() == [[2, 2, 2, 2]]
    assert LO.lookup_rows(np.array([[1, 2, 7, 7, 1, 2]], dtype=np.int32), np.array([6]), np.array([0]), np.array([2]), 3, 2, 0)[1].tolist() == [3]


def test_rule_against_transformers_prompt_lookup():
    """B = 1, from = 0, histories without a stop token.  transformers returns the continuation of the longest n-gram's FIRST match
    too; versions differ in how they cut the continuation, so only versions whose generator takes these arguments are compared"""
    cg = pytest.importorskip("transformers.generation.candidate_generator")
    gen_cls = getattr(cg, "PromptLookupCandidateGenerator", None)
    if gen_cls is None:
        pytest.skip("this transformers has no PromptLookupCandidateGenerator")
    rng = np.random.default_rng(11)
    for _ in range(200):
        n, k, N = int(rng.integers(2, 40)), int(rng.integers(1, 16)), int(rng.integers(1, 9))
        h = rng.integers(0, 3, size=n).tolist()
        try:
            g = gen_cls(num_output_tokens=k, max_matching_ngram_size=N, max_length=10 ** 6)
        except TypeError:
            pytest.skip("this transformers' PromptLookupCandidateGenerator takes other arguments")
        out = g.get_candidates(torch.tensor([h]))[0][0, n:].tolist()
        assert out == LO.lookup(h, k, N), (h, k, N)


# ---- the chains on the oracle -----------------------------------------------------------------------------------------------------
def _case(b, seed=0):
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    cond = synth.uniform(13, "cond_latents", (b, 32, dims["d_model"]), 1.0)
    codes = synth.integers(13, "content_codes", (b, 6), 256)
    return w, dims, cond, codes


_plain = {}


def plain_greedy(rep):
    """the oracle's plain greedy decoding of the case, computed once and shared (read-only)"""
    if rep not in _plain:
        w, dims, cond, codes = _case(2)
        _plain[rep] = AO.greedy(AO.BO.OracleGpt(w, dims), cond, codes, dict(suppress_tokens=SUPPRESS), rep, 16)
    return _plain[rep]


@pytest.mark.parametrize("N", [1, 2, 8])
@pytest.mark.parametrize("k", [1, 3, 15])
def test_greedy_chain_equals_plain_greedy(k, N):
    """a property of the scheme, in the oracle's own arithmetic: whatever is looked up, the tokens are plain greedy's"""
    w, dims, cond, codes = _case(2)
    for rep in (1.0, 2.0):
        r = plain_greedy(rep)
        c = LO.generate(w, dims, cond, codes, k, N, 16, kw=dict(suppress_tokens=SUPPRESS), rep=rep)
        assert np.array_equal(c["ids"], r["ids"])
        # (the latents of the tokens a row emitted: the plain loop runs both rows in one batch, the chain one row at a time)
        for b, row in enumerate(r["ids"]):
            n = int(np.nonzero(row == EOS)[0][0]) + 1 if (row == EOS).any() else len(row)
            assert float((c["latents"][b, :n] - r["latents"][b, :n]).abs().max()) < 1e-5
        assert (c["accepted"] <= c["drafted"]).all() and (c["drafted"] <= k * c["rounds"]).all() and (c["hits"] <= c["rounds"]).all()
    assert c["drafted"].sum() > 0          # three codes: something recurs


def test_onehot_rule_equals_the_rule_on_explicit_onehot_rows():
    """speculative sampling with q = one-hot: decide() of tests/spec_sample_oracle.py on explicit one-hot rows accepts x iff
    u_acc <= p(x) and otherwise draws from p with x removed -- token for token the closed form"""
    rng = np.random.default_rng(5)
    acc = rej = 0
    for t in range(400):
        Vs = 24
        s = torch.from_numpy(rng.normal(size=Vs).astype(np.float32) * 2.0)
        s[torch.from_numpy(rng.random(Vs) < 0.3)] = -LO.INF
        if not torch.isfinite(s).any():
            continue
        x = int(rng.integers(0, Vs))
        if t % 7 == 0:
            s = torch.full((Vs,), -LO.INF)
            s[x] = 1.5                                                         # p is one-hot at x itself: the residual is empty
        r, u = SO.O.rng_uniform(3, t, 1), SO.O.rng_uniform(3, t, 2)
        tok, ok, _ = SO.decide(s, torch.from_numpy(LO.onehot(x, Vs)), x, r, u)
        w, _ = SO.weights(s)
        assert ok == (float(np.float32(r)) <= (w / w.sum())[x])
        assert (tok, ok) == LO.decide_onehot(s, x, r, u)
        assert ok or tok != x or t % 7 == 0                                    # a rejected draft is not drawn again
        acc, rej = acc + ok, rej + (not ok)
    assert acc > 50 and rej > 50


def test_sampled_chain_runs_on_position_keyed_uniforms():
    w, dims, cond, codes = _case(1)
    samp = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=1.0)
    a = LO.generate(w, dims, cond, codes, 3, 2, 12, samp=samp, seed=4, kw=dict(suppress_tokens=SUPPRESS))
    b = LO.generate(w, dims, cond, codes, 3, 2, 12, samp=samp, seed=4, kw=dict(suppress_tokens=SUPPRESS))
    assert np.array_equal(a["ids"], b["ids"]) and set(a["ids"].ravel().tolist()) <= set(KEEP + (EOS,))
    assert (a["accepted"] <= a["drafted"]).all() and np.isfinite(a["floor"])


def _state(B, n0, max_new, d, em, rng):
    ids = np.ones((B, n0 + max_new + 16), dtype=np.int32)
    for b in range(B):
        ids[b, n0:n0 + em[b]] = rng.integers(0, 30, size=em[b])
    return dict(ids=ids, ids_len=n0 + np.array(em), finished=np.zeros(B, dtype=np.int32), emitted=np.array(em, dtype=np.int32),
                pending=np.full(B, -1, dtype=np.int32), toks=np.full((B, max_new), 31, dtype=np.int32),
                lats=np.zeros((B, max_new, d), dtype=np.float32), drop_target=np.zeros(B, dtype=np.int32),
                drop_assistant=np.zeros(B, dtype=np.int32), rounds=np.zeros(B, dtype=np.int32), drafted=np.zeros(B, dtype=np.int32),
                accepted=np.zeros(B, dtype=np.int32), max_new=max_new)


def test_accept_restatements_with_draft_len():
    """draft_len None or >= k: the accept steps of tests/assist_oracle.py / tests/spec_sample_oracle.py, field for field; below k: no
    more than draft_len drafts are compared or counted"""
    rng = np.random.default_rng(9)
    B, k, Vs, eos, n0, max_new, d = 4, 4, 32, 31, 5, 12, 4
    logits = rng.normal(size=(B, k + 1, Vs)).astype(np.float32) * 2.0
    logits[:, :, eos] = -20.0          # (no row stops)
    latents = rng.normal(size=(B, k + 1, d)).astype(np.float32)
    em = [1, 3, 2, max_new - 2]
    base = _state(B, n0, max_new, d, em, rng)
    drafts = logits[:, :k].argmax(-1).astype(np.int32)                          # plain argmax: every draft agrees without a penalty
    samp = dict(repetition_penalty=1.0, temperature=1.0, top_k=0, top_p=1.0)
    q = np.stack([np.stack([LO.onehot(-1, Vs)] + [LO.onehot(int(x), Vs) for x in drafts[b]]) for b in range(B)])

    def copy():
        return {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in base.items()}
    want_g, want_s = copy(), copy()
    AO.accept(want_g, k, k + 1, logits, latents, drafts, 1.0, eos)
    SO.accept(want_s, k, k + 1, logits, latents, drafts, q, samp, 2, eos)
    for dl in (None, np.full(B, k), np.full(B, k + 5)):
        got_g, got_s = copy(), copy()
        LO.accept_len(got_g, k, k + 1, logits, latents, drafts, dl, 1.0, eos)
        LO.accept_sample_len(got_s, k, k + 1, logits, latents, drafts, dl, q, samp, 2, eos)
        for n in want_g:
            assert np.array_equal(got_g[n], want_g[n]) and np.array_equal(got_s[n], want_s[n]), n
    assert want_g["accepted"].tolist() == [k, k, k, 1] and want_g["drafted"].tolist() == [k, k, k, 1]
    dl = np.array([0, 2, 9, 3])
    got_g, got_s = copy(), copy()
    LO.accept_len(got_g, k, k + 1, logits, latents, drafts, dl, 1.0, eos)
    LO.accept_sample_len(got_s, k, k + 1, logits, latents, drafts, dl, q, samp, 2, eos)
    assert got_g["drafted"].tolist() == [0, 2, k, 1] and got_g["accepted"].tolist() == [0, 2, k, 1]
    assert got_g["emitted"].tolist() == [2, 6, 2 + k + 1, max_new] and got_g["drop_target"].tolist() == [k, k - 2, 0, k - 1]
    assert got_s["drafted"].tolist() == [0, 2, k, 1] and (got_s["accepted"] <= got_s["drafted"]).all()


# ---- the kwargs ---------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("k", [0, 16, -1, 2.0, True, "5"])
def test_prompt_lookup_num_tokens_out_of_range(k):
    with pytest.raises(ValueError, match=r"prompt_lookup_num_tokens must be an int in \[1, 15\] for " + MODE):
        cpu_gpt().generate(*inputs(), do_sample=False, prompt_lookup_num_tokens=k)


@pytest.mark.parametrize("N", [0, 9, -1, 2.0, True, "2"])
def test_max_matching_ngram_size_out_of_range(N):
    with pytest.raises(ValueError, match=r"max_matching_ngram_size must be an int in \[1, 8\] for " + MODE):
        cpu_gpt().generate(*inputs(), do_sample=False, prompt_lookup_num_tokens=3, max_matching_ngram_size=N)


def test_value_errors():
    g = cpu_gpt(max_slots=64)
    cond, codes = inputs()
    with pytest.raises(ValueError, match="prompt_lookup_num_tokens and assistant_model are two draft sources"):
        g.generate(cond, codes, do_sample=False, prompt_lookup_num_tokens=3, assistant_model=ready(cpu_gpt()))
    with pytest.raises(ValueError, match="max_matching_ngram_size=2 needs prompt_lookup_num_tokens"):
        g.generate(cond, codes, do_sample=False, max_matching_ngram_size=2)
    with pytest.raises(ValueError, match="max_matching_ngram_size=2 needs prompt_lookup_num_tokens"):
        g.generate(cond, codes, do_sample=False, max_matching_ngram_size=2, assistant_model=ready(cpu_gpt()))
    with pytest.raises(ValueError, match=MODE + r": 9 items x \(prompt_lookup_num_tokens \+ 1 = 16\) rows exceed the 128 rows"):
        g.generate(*inputs(B=9), do_sample=False, prompt_lookup_num_tokens=15)
    with pytest.raises(ValueError, match=MODE + r": 2 items need 2 KV slots \(the context has 1\)"):
        cpu_gpt(max_slots=1).generate(cond, codes, do_sample=False, prompt_lookup_num_tokens=3)
    with pytest.raises(ValueError, match="speculative_sampling must be True, False or None"):
        g.generate(cond, codes, prompt_lookup_num_tokens=3, speculative_sampling=1)
    # a valid call gets as far as the engine check (no engine on this CPU-only module)
    for more in (dict(prompt_lookup_num_tokens=1), dict(prompt_lookup_num_tokens=15, max_matching_ngram_size=8),
                 dict(prompt_lookup_num_tokens=3, max_matching_ngram_size=1, repetition_penalty=2.0, no_repeat_ngram_size=2),
                 dict(prompt_lookup_num_tokens=3, do_sample=True, top_k=1), dict(prompt_lookup_num_tokens=3, assistant_model=None),
                 dict(prompt_lookup_num_tokens=3, do_sample=True, top_k=15, speculative_sampling=True, suppress_tokens=[1, 2])):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate(cond, codes, **dict(dict(do_sample=False), **more))
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):          # 8 x 16 = 128 rows fit
        g.generate(*inputs(B=8), do_sample=False, prompt_lookup_num_tokens=15)


def test_combinations_raise_by_name():
    g = cpu_gpt(max_slots=16)
    cond, codes = inputs(B=1)
    cases = [(dict(), r"sampling \(do_sample=True, top_k=0\) with " + MODE),
             (dict(do_sample=True, top_k=15), r"sampling \(do_sample=True, top_k=15\) with " + MODE),
             (dict(do_sample=False, num_beams=4), r"beam search \(num_beams=4\) with " + MODE),
             (dict(do_sample=False, num_beams=4, num_beam_groups=2, diversity_penalty=0.5), "beam groups .* with " + MODE),
             (dict(do_sample=False, top_k=4, penalty_alpha=0.6), r"contrastive search \(penalty_alpha=0.6\) with " + MODE),
             (dict(do_sample=False, guidance_scale=2.0, negative_cond_latents=cond), r"guidance_scale=2.0 with " + MODE),
             (dict(do_sample=False, num_return_sequences=3), "num_return_sequences=3 with " + MODE),
             (dict(do_sample=False, return_dict_in_generate=True, output_scores=True), "output_scores=True with " + MODE),
             (dict(do_sample=False, return_dict_in_generate=True, output_logits=True), "output_logits=True with " + MODE),
             (dict(do_sample=False, sequence_bias={(5,): 1.0}), "sequence_bias=.* is not served with " + MODE),
             (dict(do_sample=False, bad_words_ids=[[5]]), "bad_words_ids=.* is not served with " + MODE),
             (dict(do_sample=False, forced_eos_token_id=1025), "forced_eos_token_id=.* is not served with " + MODE),
             (dict(do_sample=False, renormalize_logits=True), "renormalize_logits=.* is not served with " + MODE),
             (dict(speculative_sampling=True, typical_p=0.5), "typical_p / epsilon_cutoff / eta_cutoff with " + MODE),
             (dict(speculative_sampling=True, epsilon_cutoff=0.01), "typical_p / epsilon_cutoff / eta_cutoff with " + MODE),
             (dict(speculative_sampling=True, eta_cutoff=0.01), "typical_p / epsilon_cutoff / eta_cutoff with " + MODE)]
    for kw, msg in cases:
        with pytest.raises(NotImplementedError, match=msg):
            g.generate(cond, codes, prompt_lookup_num_tokens=3, **kw)


def test_refused_paths_name_themselves():
    from genvc_amd.inference.inference_utils import synthesize_utt_streaming
    from genvc_amd.streaming import StreamSessions
    g = cpu_gpt()
    cond, codes = inputs(B=1)
    for kw in (dict(prompt_lookup_num_tokens=3, do_sample=False), dict(max_matching_ngram_size=2, do_sample=False)):
        for where, call in (("streaming (get_generator)", lambda: next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))),
                            ("grouped (generate_groups)", lambda: g.generate_groups([(cond, codes)], **kw)),
                            ("rolling (generate_rolling)", lambda: g.generate_rolling([(cond, codes)], **kw)),
                            ("session (StreamSessions, open)", lambda: StreamSessions._procs(object(), dict(kw), {}, "open")),
                            ("streaming (synthesize_utt_streaming, infer.py --streaming)",
                             lambda: synthesize_utt_streaming(None, None, None, generate_kwargs=kw))):
            with pytest.raises(NotImplementedError, match=MODE + re.escape(f" is not on the {where} path")):
                call()
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):          # the kwargs at None: these paths behave as before
        g.generate_groups([(cond, codes)], prompt_lookup_num_tokens=None, max_matching_ngram_size=None)


@pytest.mark.parametrize("off", [dict(prompt_lookup_num_tokens=None), dict(prompt_lookup_num_tokens=None, max_matching_ngram_size=None)])
def test_without_the_kwarg_the_existing_path_is_unchanged(off, monkeypatch):
    g = cpu_gpt()
    cond, codes = inputs()
    seen = {}

    class Reached(Exception):
        pass

    def start(fake, kw, fan=1):
        seen.update(kw)
        raise Reached

    monkeypatch.setattr(g, "compute_embeddings", lambda c, t: torch.ones(int(t.shape[0]), 40, dtype=torch.long))
    monkeypatch.setattr(g, "_start", start)
    monkeypatch.setattr(g, "_generate_assisted", lambda *a, **k: pytest.fail("assisted branch taken without a draft source"))
    kw = dict(do_sample=False, repetition_penalty=2.0, max_new_tokens=7, **off)
    with pytest.raises(Reached):
        g.generate(cond, codes, **kw)
    assert set(seen) == set(kw) and all(seen[k] is kw[k] for k in kw)


class StandIn:
    """an engine stand-in that plays the device's part of a lookup generation: a fixed number of tokens per round and row"""

    def __init__(self, g, per_round=(2, 4)):
        self.dims = g.dims()
        self.calls = []
        self.per_round = per_round

    def prefix_embeddings(self, cond, codes):
        return torch.zeros(cond.shape[0], cond.shape[1] + codes.shape[1] + 2, cond.shape[2])

    def prefill(self, slots, prefix, want_outputs=True, n_cached=0):
        self.calls.append(("prefill", tuple(slots.tolist()), tuple(prefix.shape), want_outputs, n_cached))

    def generate_assisted(self, *a, **k):
        pytest.fail("the draft-model entry was called for a lookup generation")

    def generate_lookup(self, slots, st, params, n_rounds, max_keys, max_ngram, proc=None, k=None, sampling=False):
        self.calls.append(("generate_lookup", n_rounds, k, max_keys, max_ngram, proc is not None, params.top_k, sampling))
        for b in range(st.B):
            if not st.opened:
                st.toks[b, 0] = 7
                st.emitted[b] = 1
            for _ in range(n_rounds):
                if st.finished[b]:
                    continue
                n = min(self.per_round[b % len(self.per_round)], k + 1, st.max_new - int(st.emitted[b]))
                st.toks[b, int(st.emitted[b]):int(st.emitted[b]) + n] = 7
                st.emitted[b] += n
                st.rounds[b] += 1
                st.finished[b] = int(st.emitted[b] >= st.max_new)
        st.opened = True

    def health(self):
        self.calls.append(("health",))

    def reset(self, slots):
        self.calls.append(("reset",))


def test_host_loop_through_a_stand_in():
    import genvc_amd.engine as E
    import genvc_amd.layers.gpt as G
    g = cpu_gpt()
    g.engine = StandIn(g)
    cond, codes = inputs(B=2, Tc=5)
    n0 = 32 + 5 + 2 + 1
    out = g.generate(cond, codes, do_sample=False, prompt_lookup_num_tokens=3, max_matching_ngram_size=4, max_new_tokens=12,
                     no_repeat_ngram_size=2, group=8)
    assert out.shape == (2, 12) and bool((out == 7).all()) and g.last_latents.shape == (2, 12, D)
    assert set(g.last_assist_stats) == {"rounds", "drafted", "accepted"}
    calls = [c for c in g.engine.calls if c[0] == "generate_lookup"]
    assert [c[1] for c in calls] == [2, 2, 2] and all(c[2] == 3 and c[4] == 4 for c in calls)
    assert all(c[5:] == (True, 1, False) for c in calls)
    assert [c[3] for c in calls] == [n0 + 5 + 3, n0 + 11 + 3, n0 + 11 + 3]          # as the draft-model loop counts them
    assert g.engine.calls[0][:2] == ("prefill", (0, 1)) and g.engine.calls.count(("health",)) == 3
    # N defaults to 2; the sampled mode passes the call's top_k on
    g.engine.calls.clear()
    g.generate(cond, codes, prompt_lookup_num_tokens=3, speculative_sampling=True, top_k=15, max_new_tokens=12)
    calls = [c for c in g.engine.calls if c[0] == "generate_lookup"]
    assert calls and all(c[4] == 2 and c[5:] == (False, 15, True) for c in calls)
    assert E.MAX_LOOKUP_NGRAM == 8 and E.MAX_LOOKUP_HISTORY == 2048 and G.LOOKUP_KWARGS == ("prompt_lookup_num_tokens", "max_matching_ngram_size")


def test_drafts_shrink_at_the_end_of_the_position_table():
    g = cpu_gpt(max_mel_tokens=30)
    g.engine = StandIn(g, per_round=(8,))
    out = g.generate(*inputs(B=1), do_sample=False, prompt_lookup_num_tokens=7, group=1)
    assert out.shape == (1, 27)
    assert [c[2] for c in g.engine.calls if c[0] == "generate_lookup"] == [7, 7, 7, 6]          # as with a draft model
    with pytest.raises(ValueError, match=MODE + ".*leaves no room for a draft"):
        g.generate(*inputs(B=1), do_sample=False, prompt_lookup_num_tokens=7, max_new_tokens=32)


def test_history_bound():
    g = cpu_gpt(max_mel_tokens=4000)
    g.engine = StandIn(g)
    with pytest.raises(ValueError, match=MODE + ": max_new_tokens=2033 is above the 2032 generated ids a lookup searches"):
        g.generate(*inputs(B=1), do_sample=False, prompt_lookup_num_tokens=3, max_new_tokens=2033)


def test_harness_passes_the_kwargs_through():
    from genvc_amd.inference import inference_utils as IU
    seen = []

    class M:
        device = "cpu"
        content_sample_rate = 16000
        hifigan = None
        config = type("C", (), dict(audio=type("A", (), dict(sample_rate=24000))(), top_p=0.85, top_k=15, temperature=0.75,
                                    length_penalty=1.0, repetition_penalty=10.0,
                                    model_args=type("MA", (), dict(gpt_code_stride_len=1024))()))()

        def get_gpt_cond_latents(self, audio, sr):
            return torch.zeros(1, 32, D)

        class content_extractor:
            @staticmethod
            def extract_content_features(seg):
                return torch.zeros(1, 4, 8)

        class content_dvae:
            @staticmethod
            def get_codebook_indices(feat):
                return torch.zeros(1, 4, dtype=torch.long)

        class gpt:
            stop_audio_token = 1025
            last_latents = None

            @staticmethod
            def generate(cond, codes, **kw):
                seen.append(kw)
                M.gpt.last_latents = torch.zeros(1, 3, D)
                return torch.tensor([[5, 6, 1025]])

    gkw = dict(prompt_lookup_num_tokens=4, max_matching_ngram_size=3, do_sample=False)
    IU.synthesize_utt(M(), torch.zeros(1, 16000 * 2 + 100), torch.zeros(1, 24000), seg_len=1.0, generate_kwargs=gkw)
    assert len(seen) == 3
    for kw in seen:
        assert kw["prompt_lookup_num_tokens"] == 4 and kw["max_matching_ngram_size"] == 3 and kw["do_sample"] is False


def _infer(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--device", "cpu", *flags], capture_output=True, text=True,
                          env=env, cwd=ROOT)


def test_infer_flags():
    r = _infer("--streaming", "--prompt_lookup_num_tokens", "3")
    assert r.returncode != 0 and "--prompt_lookup_num_tokens is not on the streaming path (--streaming)" in r.stderr
    r = _infer("--max_matching_ngram_size", "3")
    assert r.returncode != 0 and "--max_matching_ngram_size needs --prompt_lookup_num_tokens" in r.stderr
    r = _infer("--prompt_lookup_num_tokens", "16")
    assert r.returncode != 0 and "--prompt_lookup_num_tokens must be in [1, 15]" in r.stderr
    r = _infer("--prompt_lookup_num_tokens", "3", "--num_beams", "4")
    assert r.returncode != 0 and "--prompt_lookup_num_tokens does not combine with --num_beams" in r.stderr
    r = _infer("--synthetic", "--prompt_lookup_num_tokens", "3", "--assistant_layers", "2")
    assert r.returncode != 0 and "two draft sources" in r.stderr


def test_new_symbols_declared_and_exported():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    assert all(len(_lib._SIGNATURES[s][1]) == n for s, n in zip(SYMBOLS, (8, 11, 13, 14)))          # the argument counts of the header
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s
