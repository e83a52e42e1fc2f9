"""GPU: prompt-lookup assisted decoding (GPT.generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=N); include/genvc_hip.h:
gvc_spec_lookup, gvc_spec_accept_len, gvc_spec_accept_sample_len, gvc_gpt_generate_lookup) against tests/lookup_oracle.py.
1. the lookup kernel alone on crafted id rows: v_toks, draft_len and the one-hot rows exactly;  2. the accept steps with a draft count
   per row on the parameter cases of tests/test_gpu_assisted.py and tests/test_gpu_spec_sample.py, and a null count against the
   entries without one, bit for bit;  3. whole generations: greedy ids against plain greedy and the oracle, sampled ids against the
   CPU chain, and the counters of both, on margin-screened cases (every screen is asserted on the CPU before any GPU work)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assist_oracle as AO                    # noqa: E402
import lookup_oracle as LO                    # noqa: E402
import spec_sample_oracle as SO               # noqa: E402
import test_gpu_assisted as TA                # noqa: E402  (its accept cases, model builders and screen)
import test_gpu_spec_sample as TS             # noqa: E402  (its accept cases)
from genvc_amd import config as gcfg          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026
TINY, FULL2 = TA.TINY, TA.FULL2
TOL = 1e-4
MARGIN, LOGIT_SCREEN = TS.MARGIN, TS.LOGIT_SCREEN
KEEP = (7, 300, 1000)                         # the codes a generation may use besides the stop token: n-grams must recur
SUPPRESS = [i for i in range(V) if i not in KEEP + (EOS,)]
KW = dict(suppress_tokens=SUPPRESS)


# ---- 1. the lookup kernel ---------------------------------------------------------------------------------------------------------------
def planted(idx, n, total=300):
    """`total` distinct codes whose last n ids occur once more, at index idx (idx = total - 1 - n: the last n + 1 ids are one code)"""
    h = list(range(10, 10 + total))
    if idx + n > total - n:
        h[idx:] = [999] * (total - idx)
    else:
        h[idx:idx + n] = h[total - n:]
    return h


CRAFTED = [[5], [5, 5], [1, 2, 3, 4], [1, 2, 9, 8, 1, 2, 7, 6, 1, 2], [2, 5, 5, 1, 2, 6, 6, 1, 2], [4, 1, 2, 3, 1, 2], [1, 2, 1, 2, 1, 2],
           [3, 3, 3]]


def run_lookup(hists, k, N, start=3, finished=None, q=False, pad=None):
    """the kernel on one state: row b's ids are `start` placeholders (pad[b], default 1) and hists[b].  -> (v_toks [B, k + 1], draft_len
    [B], q [B, k + 1, V] or None) from the device, and the same from tests/lookup_oracle.py"""
    from genvc_amd.engine import AssistedState, spec_lookup
    B = len(hists)
    finished = finished or [0] * B
    st = AssistedState(torch.ones(B, start, dtype=torch.int32, device=DEV), k, max(len(h) for h in hists), EOS, V, 8, latents=False)
    ids = st.ids.cpu().numpy()
    for b, h in enumerate(hists):
        if pad is not None:
            ids[b, :start] = pad[b]
        ids[b, start:start + len(h)] = h
    ids_len = np.array([start + len(h) for h in hists], dtype=np.int32)
    pending = np.array([h[-1] for h in hists], dtype=np.int32)
    st.ids.copy_(torch.from_numpy(ids))
    st.ids_len.copy_(torch.from_numpy(ids_len))
    st.finished.copy_(torch.tensor(finished, dtype=torch.int32))
    st.pending.copy_(torch.from_numpy(pending))
    st.draft_len.fill_(-7)
    qd = torch.full((B, k + 1, V), 7.0, device=DEV) if q else None
    spec_lookup(st, k, N, start, qd)
    got = (st.v_toks.view(-1)[:B * (k + 1)].view(B, k + 1).cpu().numpy(), st.draft_len.cpu().numpy(), qd.cpu().numpy() if q else None)
    return got, LO.lookup_rows(ids, ids_len, finished, pending, k, N, start, vocab=V if q else None)


@pytest.mark.parametrize("k,N", [(3, 2), (1, 1), (15, 8), (1, 8), (15, 1)])
def test_lookup_crafted_rows(k, N):
    """a history shorter than n + 1; only the suffix itself matches; two matches; a longer n against an earlier short match; the
    continuation cut at the end; a periodic history; all as one batch of rows with their own lengths"""
    (v, dl, _), (wv, wdl, _) = run_lookup(CRAFTED, k, N)
    print(f"k {k} N {N}: draft_len {dl.tolist()}")
    assert np.array_equal(dl, wdl) and np.array_equal(v, wv)
    if (k, N) == (3, 2):          # what the rows were crafted for
        assert dl.tolist() == [0, 1, 0, 3, 3, 3, 3, 1]
        assert v[3].tolist() == [2, 9, 8, 1] and v[4].tolist() == [2, 6, 6, 1] and v[5].tolist() == [2, 3, 1, 2]
        assert v[6].tolist() == [2, 1, 2, 1] and v[2].tolist() == [4, 4, 4, 4]


def test_lookup_never_searches_before_from():
    """the placeholders before `from` hold the suffix (in row 1 with a continuation that lies before `from` too): no match"""
    hists = [[7, 7, 1, 2], [6, 7, 1, 2]]
    (v, dl, _), (wv, wdl, _) = run_lookup(hists, 3, 2, start=3, pad=[[9, 1, 2], [1, 2, 5]])
    assert dl.tolist() == [0, 0] and np.array_equal(dl, wdl) and np.array_equal(v, wv)
    # the same ids with from = 0 do match: the rule, not the data, keeps them out
    (v, dl, _), (wv, wdl, _) = run_lookup([[9, 1, 2, 7, 7, 1, 2], [1, 2, 5, 6, 7, 1, 2]], 3, 2, start=0)
    assert dl.tolist() == [3, 3] and np.array_equal(v, wv)


@pytest.mark.parametrize("N", [1, 2, 8])
def test_lookup_strided_loop_boundaries(N):
    """300 codes whose only match starts at index 255 (the last start of the threads' first pass), 256 (thread 0's second pass) and
    299 - n (the last start that leaves a continuation)"""
    hists = [planted(255, N), planted(256, N), planted(299 - N, N)]
    (v, dl, _), (wv, wdl, _) = run_lookup(hists, 5, N)
    assert np.array_equal(dl, wdl) and np.array_equal(v, wv)
    assert dl.tolist() == [5, 5, 1]
    assert v[0, 1:].tolist() == hists[0][255 + N:260 + N] and v[1, 1:].tolist() == hists[1][256 + N:261 + N] and v[2, 1] == hists[2][299]


@pytest.mark.parametrize("k,N", [(3, 2), (15, 8), (1, 1)])
def test_lookup_batch_with_a_finished_row_and_onehot_rows(k, N):
    """B = 3, three lengths, row 1 finished: draft_len 0 and only pending tokens there; the one-hot rows entry by entry at vocab 1026
    (as the accept step reads them: warped scores, 0 at the token and -inf elsewhere -- probability exactly 1 and 0), row 0 of every
    stream and the finished stream's rows untouched"""
    hists = [[1, 2, 9, 8, 1, 2, 7, 6, 1, 2], [4, 4, 4, 4, 4], planted(256, 2, total=270)]
    (v, dl, q), (wv, wdl, wq) = run_lookup(hists, k, N, finished=[0, 1, 0], q=True)
    assert np.array_equal(dl, wdl) and np.array_equal(v, wv) and dl[1] == 0 and v[1].tolist() == [4] * (k + 1) and dl[0] > 0
    written = ~np.isnan(wq)
    assert np.array_equal(q[written], wq[written]) and (q[~written] == 7.0).all()
    assert not written[:, 0].any() and not written[1].any() and written[0, 1:].all() and written[2, 1:].all()
    for b in (0, 2):
        for j in range(1, k + 1):
            w, _ = SO.weights(torch.from_numpy(q[b, j]))
            p = w / w.sum()
            want = np.zeros(V)
            want[v[b, j]] = 1.0
            assert np.array_equal(p, want)


def test_lookup_refuses_bad_arguments_on_the_host():
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import AssistedState, spec_lookup
    st = AssistedState(torch.ones(2, 4, dtype=torch.int32, device=DEV), 3, 12, EOS, V, 8, latents=False)
    st.draft_len.fill_(-7)
    for k, N, start in ((0, 2, 4), (16, 2, 4), (3, 0, 4), (3, 9, 4), (3, 2, -1)):
        with pytest.raises(GenvcHipError):
            spec_lookup(st, k, N, start)
    big = AssistedState(torch.ones(1, 4, dtype=torch.int32, device=DEV), 3, 2040, EOS, V, 8, latents=False)
    with pytest.raises(GenvcHipError, match="exceeds 2048"):
        spec_lookup(big, 3, 2, 4)          # 2040 + 16 ids behind `from`
    spec_lookup(big, 3, 2, 12)             # 2048 fit
    torch.cuda.synchronize()
    assert st.draft_len.tolist() == [-7, -7]          # nothing was launched


# ---- 2. the accept steps with a draft count per row -----------------------------------------------------------------------------------------
def _null_call(fn, st, k, appended, logits, latents, drafts, extra, params, proc):
    """the new entry with a NULL draft_len, called directly"""
    from genvc_amd._lib import check, ptr, stream
    check(fn(C.byref(st.c), k, appended, ptr(logits), ptr(latents), ptr(drafts), drafts.shape[1], None, *extra, C.byref(params),
             None if proc is None else C.byref(proc), stream()), "accept_len")


ACC_LENS = [[0, 1, TA.K_ACC, TA.K_ACC + 3, 2, TA.K_ACC - 1, 1], [TA.K_ACC, 0, 2, 1, 3, 9, 0]]          # below, at and above k


@pytest.mark.parametrize("kw", [{}, {"min_new_tokens": 3}, {"suppress_tokens": [3, 500, 1000]}, {"no_repeat_ngram_size": 2}],
                         ids=["plain", "min_new_tokens", "suppress_tokens", "ngram"])
@pytest.mark.parametrize("rep", [1.0, 2.0])
def test_accept_len_matches_numpy(rep, kw):
    from genvc_amd._lib import lib
    from genvc_amd.engine import logits_processors, sample_params, spec_accept
    k = TA.K_ACC
    params = sample_params(dict(repetition_penalty=rep, temperature=1.0, top_p=1.0, top_k=1), V, EOS)
    proc = logits_processors(kw, TA.N0, V, sampling=False)
    for dl in ACC_LENS:
        st, ref, logits, latents, drafts = TA.accept_case(rep, kw)
        spec_accept(st, k, k + 1, logits.to(DEV), latents.to(DEV), torch.from_numpy(drafts).to(DEV), params, proc=proc,
                    draft_len=torch.tensor(dl, dtype=torch.int32, device=DEV))
        LO.accept_len(ref, k, k + 1, logits.numpy(), latents.numpy(), drafts, np.array(dl), rep, EOS, kw, TA.N0)
        TA.compare_state(st, ref)
        budget = [min(k, TA.MAX_NEW - e - 1) for e, _, _, _ in TA.ACC_ROWS]
        live = [not r[3] for r in TA.ACC_ROWS]
        assert ref["drafted"].tolist() == [min(b, d) if on else 0 for b, d, on in zip(budget, dl, live)]
    assert ref["drafted"][1] == 0 and ref["emitted"][1] == TA.ACC_ROWS[1][0] + 1          # no draft: one target token, the round counted
    # a null count: the entry without one, bit for bit
    st, ref, logits, latents, drafts = TA.accept_case(rep, kw)
    st2 = TA.accept_case(rep, kw)[0]
    spec_accept(st, k, k + 1, logits.to(DEV), latents.to(DEV), torch.from_numpy(drafts).to(DEV), params, proc=proc)
    _null_call(lib().gvc_spec_accept_len, st2, k, k + 1, logits.to(DEV), latents.to(DEV), torch.from_numpy(drafts).to(DEV), (), params, proc)
    for name in TS.STATE:
        assert torch.equal(getattr(st, name), getattr(st2, name)), name


SAMPLE_LENS = [[0, 2, TS.K_ACC, 9, 3, 1, 4, TS.K_ACC], [TS.K_ACC, 0, 1, 2, 0, 7, 2, 3], [1, TS.K_ACC, 0, 3, 2, 2, TS.K_ACC + 1, 0]]


@pytest.mark.parametrize("kw", [(), (("min_new_tokens", 3),), (("no_repeat_ngram_size", 2),), (("min_p", 0.05),)],
                         ids=["plain", "min_new_tokens", "ngram", "min_p"])
@pytest.mark.parametrize("rep", [1.0, 2.0])
@pytest.mark.parametrize("top_k,top_p", [(15, 0.85), (0, 1.0), (50, 0.7)])
def test_accept_sample_len_matches_oracle(top_k, top_p, rep, kw):
    """the 24 cases of tests/test_gpu_spec_sample.py with draft counts below, at and above k.  A clamped row draws its last token from
    p where the unclamped case tested a draft, so the margins are screened again: the first count pattern whose decisions all clear
    MARGIN is used, and the screen is asserted"""
    from genvc_amd._lib import lib
    from genvc_amd.engine import logits_processors, sample_params, spec_accept_sample
    c = TS.accept_case(top_k, top_p, rep, kw)
    k = TS.K_ACC

    def fresh():
        return {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in c["base"].items()}
    for dl in SAMPLE_LENS:
        ref = fresh()
        out = LO.accept_sample_len(ref, k, k + 1, c["logits"].numpy(), c["latents"].numpy(), c["drafts"], np.array(dl), c["q"], c["samp"],
                                   c["seed"], EOS, c["kw"], TS.N0)
        if min(out["margins"]) > MARGIN:
            break
    print(f"draft_len {dl}: smallest margin {min(out['margins']):.3e}, drafted {ref['drafted'].tolist()} accepted {ref['accepted'].tolist()}")
    assert min(out["margins"]) > MARGIN, "no count pattern clears the margins"
    budget = [min(k, TS.MAX_NEW - e - 1) for e in TS.EMITTED]
    assert ref["drafted"].tolist() == [0 if f else min(b, d) for b, d, f in zip(budget, dl, TS.FINISHED)]
    assert any(d < b for b, d, f in zip(budget, dl, TS.FINISHED) if not f) and any(d > k for d in dl)
    params = sample_params(c["samp"], V, EOS, c["seed"])
    proc = logits_processors(c["kw"], TS.N0, V, sampling=True)
    args = (c["logits"].to(DEV), c["latents"].to(DEV), torch.from_numpy(c["drafts"]).to(DEV), torch.from_numpy(c["q"]).to(DEV))
    st = TS.make_state(c["base"], k)
    spec_accept_sample(st, k, k + 1, *args, params, proc=proc, draft_len=torch.tensor(dl, dtype=torch.int32, device=DEV))
    TS.compare_state(st, ref)
    # a null count: the entry without one, bit for bit (state and warped rows)
    st1, st2 = TS.make_state(c["base"], k), TS.make_state(c["base"], k)
    p1 = spec_accept_sample(st1, k, k + 1, *args, params, proc=proc)
    p2 = torch.zeros_like(p1)
    _null_call(lib().gvc_spec_accept_sample_len, st2, k, k + 1, args[0], args[1], args[2], (args[3].data_ptr(), p2.data_ptr()), params, proc)
    TS.compare_state(st1, c["ref"])
    for name in TS.STATE:
        assert torch.equal(getattr(st1, name), getattr(st2, name)), name
    assert torch.equal(p1, p2)


# ---- 3. whole generations -------------------------------------------------------------------------------------------------------------------
_cpu = {}


def plain_oracle(args, seed, b, rep, max_new):
    """plain greedy decoding on the CPU oracle, computed once and shared (read-only)"""
    key = ("plain", id(args), seed, b, rep, max_new)
    if key not in _cpu:
        dims = gcfg.gpt_dims(args)
        cond, codes = TA.inputs(dims, b)
        _cpu[key] = AO.greedy(AO.BO.OracleGpt(TA.weights(args, seed), dims), cond, codes, KW, rep, max_new)
    return _cpu[key]


def chain(args, seed, b, k, N, max_new, rep=1.0, samp=None, rng=0):
    """the CPU round chain of one case, computed once and shared (read-only)"""
    key = ("chain", id(args), seed, b, k, N, max_new, rep, repr(samp), rng)
    if key not in _cpu:
        dims = gcfg.gpt_dims(args)
        cond, codes = TA.inputs(dims, b)
        _cpu[key] = LO.generate(TA.weights(args, seed), dims, cond, codes, k, N, max_new, samp=samp, seed=rng, kw=KW, rep=rep,
                                logit_screen=LOGIT_SCREEN, logit_tol=TOL)
    return _cpu[key]


def make_gpt(args, seed, max_new):
    g = TA.make_gpt(args, seed)
    g.max_gen_mel_tokens = max_new
    return g


def stats_of(g):
    return {n: t.cpu().numpy() for n, t in g.last_assist_stats.items()}


def latent_err(g, ids, want):
    lens = TA.row_lengths(ids)
    lat = g.last_latents.cpu()
    assert lat.shape[:2] == ids.shape
    return max(float((lat[i, :n] - want[i, :n]).abs().max()) for i, n in enumerate(lens))


# (name, model, model seed, streams, repetition penalty, max_new, [(k, N) ...]): model seeds found on the CPU -- the oracle's plain greedy
# margins clear the 2e-3 logit screen times the repetition penalty, and the chain at the first (k, N) drafts and accepts in every row
GREEDY_CASES = [("tiny", TINY, 0, 1, 1.0, 24, [(3, 2), (1, 1), (15, 8)]), ("tiny", TINY, 0, 2, 1.0, 24, [(3, 2), (7, 1), (15, 8)]),
                ("tiny-rep", TINY, 5, 2, 2.0, 24, [(3, 2), (5, 8)]), ("full2", FULL2, 0, 1, 1.0, 16, [(3, 2), (15, 8)]),
                ("full2", FULL2, 0, 2, 1.0, 16, [(3, 2), (7, 1)]), ("full2-rep", FULL2, 0, 2, 2.0, 16, [(3, 2)])]


@pytest.mark.parametrize("name,args,seed,b,rep,max_new,kns", GREEDY_CASES, ids=[f"{c[0]}-B{c[3]}" for c in GREEDY_CASES])
def test_lookup_greedy_equals_plain_greedy(name, args, seed, b, rep, max_new, kns):
    r = plain_oracle(args, seed, b, rep, max_new)
    TA.screen(r, rep)
    chains = [chain(args, seed, b, k, N, max_new, rep) for k, N in kns]
    c0 = chains[0]
    print(f"oracle: ids {r['ids'].tolist()}; chain at {kns[0]}: rounds {c0['rounds'].tolist()} drafted {c0['drafted'].tolist()} accepted "
          f"{c0['accepted'].tolist()}")
    assert (c0["drafted"] > 0).all() and (c0["accepted"] > 0).all()
    assert all(np.array_equal(c["ids"], r["ids"]) for c in chains)
    g = make_gpt(args, seed, max_new)
    cond, codes = TA.inputs(gcfg.gpt_dims(args), b)
    cond, codes = cond.to(DEV), codes.to(DEV)
    call = dict(do_sample=False, repetition_penalty=rep, **KW)
    plain = g.generate(cond, codes, **call).cpu().numpy()
    assert not hasattr(g, "last_assist_stats")
    lat_plain = g.last_latents.clone()
    assert np.array_equal(plain, r["ids"])
    for (k, N), c in zip(kns, chains):
        ids = g.generate(cond, codes, prompt_lookup_num_tokens=k, max_matching_ngram_size=N, **call).cpu().numpy()
        s = stats_of(g)
        print(f"  k {k} N {N}: rounds {s['rounds'].tolist()} drafted {s['drafted'].tolist()} accepted {s['accepted'].tolist()}")
        if name.startswith("full2"):
            assert g.engine.decode_variant() == 5          # b * (k + 1) <= 16 rows: the one-launch rows step verified them
        assert np.array_equal(ids, plain) and np.array_equal(ids, r["ids"])
        for n in ("rounds", "drafted", "accepted"):
            assert np.array_equal(s[n], c[n]), n
        assert all(t.dtype == torch.int64 and tuple(t.shape) == (b,) for t in g.last_assist_stats.values())
        err = latent_err(g, ids, r["latents"])
        print(f"  latent err {err:.3e}")
        assert err < TOL
    again = g.generate(cond, codes, **call)
    assert np.array_equal(again.cpu().numpy(), plain) and torch.equal(g.last_latents, lat_plain)          # the plain call is unchanged
    g.engine.health()
    TA.close(g)


def test_a_row_ends_inside_a_round_while_the_other_goes_on():
    """TINY seed 0, B = 2: the oracle's row 1 stops with its 9th token, row 0 with its 11th; with k = 3 row 1's last round emits fewer
    tokens than it verified while row 0 runs one round more"""
    r = plain_oracle(TINY, 0, 2, 1.0, 24)
    TA.screen(r, 1.0)
    assert TA.row_lengths(r["ids"]) == [11, 9]
    c = chain(TINY, 0, 2, 3, 2, 24)
    assert c["rounds"].tolist() == [6, 5] and (c["accepted"] > 0).all()
    g = make_gpt(TINY, 0, 24)
    cond, codes = TA.inputs(gcfg.gpt_dims(TINY), 2)
    for group in (16, 1):
        ids = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False, prompt_lookup_num_tokens=3, group=group, **KW).cpu().numpy()
        s = stats_of(g)
        assert np.array_equal(ids, r["ids"]) and ids.shape[1] == 11 and (ids[1, 9:] == EOS).all()
        assert all(np.array_equal(s[n], c[n]) for n in ("rounds", "drafted", "accepted"))
    TA.close(g)


SAMP = dict(top_k=3, top_p=0.85, temperature=0.85, repetition_penalty=2.0)
# (name, model, model seed, streams, k, N, max_new, the call's RNG seed).  top_k = 3 of the four ids the suppression leaves, so TopK decides
# in every row.  The RNG seeds are the first from 0 that pass the screen of tests/lookup_oracle.py: generate (need = MARGIN) with a chain
# that drafts and accepts in every row: every decision keeps a margin above MARGIN when the logits move by up to LOGIT_SCREEN (draws from a
# warped row, accept tests) or by up to TOL (residual draws, TopK's last gap, TopP's cut), the split of tests/test_gpu_spec_sample.py
SAMPLE_CASES = [("tiny", TINY, 0, 1, 3, 2, 16, 0), ("tiny", TINY, 0, 2, 3, 2, 16, 7), ("full2", FULL2, 0, 1, 7, 2, 12, 3),
                ("full2", FULL2, 0, 2, 7, 2, 12, 3)]


@pytest.mark.parametrize("name,args,seed,b,k,N,max_new,rng", SAMPLE_CASES, ids=[f"{c[0]}-B{c[3]}" for c in SAMPLE_CASES])
def test_lookup_sampled_matches_cpu_chain(name, args, seed, b, k, N, max_new, rng):
    c = chain(args, seed, b, k, N, max_new, samp=SAMP, rng=rng)
    print(f"chain: ids {c['ids'].tolist()} rounds {c['rounds'].tolist()} drafted {c['drafted'].tolist()} accepted {c['accepted'].tolist()}, "
          f"smallest margin less the logit allowance {c['floor']:.3e}")
    assert c["floor"] > MARGIN, "the case is not margin-screened"
    assert (c["drafted"] > 0).all() and (c["accepted"] > 0).all()
    g = make_gpt(args, seed, max_new)
    cond, codes = TA.inputs(gcfg.gpt_dims(args), b)
    cond, codes = cond.to(DEV), codes.to(DEV)
    plain = g.generate(cond, codes, seed=rng, **SAMP, **KW)
    call = dict(prompt_lookup_num_tokens=k, max_matching_ngram_size=N, speculative_sampling=True, seed=rng, **SAMP, **KW)
    ids = g.generate(cond, codes, **call).cpu().numpy()
    s = stats_of(g)
    print(f"device: ids {ids.tolist()} stats {({n: v.tolist() for n, v in s.items()})}")
    if name == "full2":
        assert g.engine.decode_variant() == 5
    assert np.array_equal(ids, c["ids"])
    for n in ("rounds", "drafted", "accepted"):
        assert np.array_equal(s[n], c[n]), n
    err = latent_err(g, ids, c["latents"])
    print(f"latent err {err:.3e}")
    assert err < TOL
    # rounds split over calls continue exactly (position-keyed uniforms), and the plain sampled call is what it was
    many = g.generate(cond, codes, group=1, **call).cpu().numpy()
    assert np.array_equal(many, ids) and all(np.array_equal(stats_of(g)[n], s[n]) for n in s)
    assert torch.equal(plain, g.generate(cond, codes, seed=rng, **SAMP, **KW))
    g.engine.health()
    TA.close(g)


def test_plain_one_stream_calls_around_a_lookup_call():
    """a plain one-stream generate leaves a deferred token in its slot; the lookup call settles it, and the plain call afterwards
    returns what it returned before"""
    r = plain_oracle(TINY, 0, 1, 1.0, 24)
    g = make_gpt(TINY, 0, 24)
    cond, codes = TA.inputs(gcfg.gpt_dims(TINY), 1)
    cond, codes = cond.to(DEV), codes.to(DEV)
    first = g.generate(cond, codes, do_sample=False, **KW)
    assert g.engine.decode_variant() == 3
    lat1 = g.last_latents.clone()
    ids = g.generate(cond, codes, do_sample=False, prompt_lookup_num_tokens=5, **KW)
    assert torch.equal(ids, first) and np.array_equal(ids.cpu().numpy(), r["ids"])
    again = g.generate(cond, codes, do_sample=False, **KW)
    assert torch.equal(first, again) and torch.equal(lat1, g.last_latents)
    TA.close(g)
