"""GPU: sequence_bias / bad_words_ids / forced_eos_token_id / renormalize_logits on the sampler kernels (include/genvc_hip.h:
gvc_logits_bias, gvc_sample_bias, gvc_gpt_generate_bias) against tests/bias_oracle.py -- the oracle's GPT forward followed by the
installed transformers' own SequenceBias / NoBadWords / ForcedEOSToken / LogitNormalization objects, executed at their places in HF's
list.  Shapes, tolerances and the margin screen are those of tests/test_gpu_scores.py and tests/test_gpu_cfg.py: TINY_MODEL_ARGS, B = 2,
12 new tokens, 1e-4 on a logit times what the chain does to an error.  The biased and banned sequences are constructed from the
unbiased oracle run, so every case provably fires, and each is compared step by step with the oracle teacher-forced with the device's
tokens."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bias_oracle as BI                      # noqa: E402
import test_gpu_cfg as TG                     # noqa: E402
import test_gpu_scores as TS                  # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V, MAX_NEW, TOL = TS.EOS, TS.V, TS.MAX_NEW, TS.TOL
TINY = gcfg.TINY_MODEL_ARGS
BOTH = TS.BOTH
NINF = -float("inf")
stacked, want, compare = TS.stacked, TS.want, TS.compare


# ---- 4. gvc_sample_bias on crafted rows ----------------------------------------------------------------------------------------------
PLEN = 6
CRAFT_KW = dict(sequence_bias={(7,): -1.0, (30, 31, 40): 3.0, (31, 40): 0.5}, bad_words_ids=[[EOS], [50, 51], [33, 50, 53]])
CRAFT_TAILS = [[7, 9], [30, 31], [30, 32], [33, 50]]
CRAFT_WANT = [20, 40, 51, 52]


def crafted():
    """B = 4 rows of logits and ids (prompt 1 1 1 1 1 1024, two generated ids), repetition penalty 2, every row's winner ahead by 0.5
    or more except row 0, which is exact arithmetic:
    row 0  token 7 is in the row (seen) at +0.5 with bias -1.0: (0.5 - 1.0) * 2 = -1.0 against the unseen 20 at -0.9 -> 20.  With the
           bias behind the penalty 7 would score 0.25 - 1.0 = -0.75 and win.
    row 1  tail 30 31 hits (30, 31, 40) and (31, 40): 40 scores 1.0 + 3.5 against 41 at 2.0 -> 40
    row 2  tail 30 32 misses both by one id: 40 stays at 1.0; 51 at 2.6 is not banned (the tail is not 50) -> 51
    row 3  tail 33 50 hits [50, 51] and [33, 50, 53]: 51 at 90 and 53 at 65 are banned, 52 at 60 -> 52 (far ahead: the sampling kernel
           draws it at top_k = 3 too, as it draws 51 without the bans)"""
    lg = torch.full((4, V), -5.0)
    lg[0, 7], lg[0, 20] = 0.5, -0.9
    lg[1, 40], lg[1, 41] = 1.0, 2.0
    lg[2, 40], lg[2, 41], lg[2, 51] = 1.0, 2.0, 2.6
    lg[3, 51], lg[3, 53], lg[3, 52] = 90.0, 65.0, 60.0
    ids = torch.ones(4, PLEN + 2 + 4, dtype=torch.int32)
    ids[:, PLEN - 1] = 1024
    ids[:, PLEN:PLEN + 2] = torch.tensor(CRAFT_TAILS, dtype=torch.int32)
    return lg, ids


def test_sample_bias_on_crafted_rows():
    from genvc_amd.engine import GptEngine, logits_bias, sample_params
    lg, ids = crafted()
    chain = BI.hf_chain(CRAFT_KW, PLEN, EOS, 2.0, MAX_NEW)
    hf = BI.run_chain(chain, ids[:, :PLEN + 2].long(), lg)
    assert hf.argmax(-1).tolist() == CRAFT_WANT
    top2 = torch.topk(hf, 2, -1)[0]
    assert bool(((top2[:, 0] - top2[:, 1])[1:] >= 0.5).all()) and float(hf[0, 7]) == -1.0
    eng = GptEngine(gcfg.gpt_dims(TINY), max_slots=2)
    bias = logits_bias(CRAFT_KW, PLEN, MAX_NEW, V, EOS)
    assert (bias.n_bias, bias.n_ban) == (3, 2)
    greedy = sample_params(dict(repetition_penalty=2.0, temperature=1.0, top_p=1.0, top_k=1), V, EOS, seed=3)
    keyed = [dict(repetition_penalty=2.0, temperature=1.0, top_p=1.0, top_k=k, seed=3, rng_row=r, rng_step0=0) for r, k in enumerate((1, 1, 1, 3))]
    for what, rows in (("argmax kernel", None), ("sampling kernel", keyed)):
        d_ids = ids.to(DEV)
        d_len = torch.full((4,), PLEN + 2, device=DEV, dtype=torch.int32)
        fin = torch.zeros(4, device=DEV, dtype=torch.int32)
        tok = eng.sample_bias(lg.to(DEV), d_ids, d_len, fin, greedy, bias, 0, rows=rows).cpu().tolist()
        print(f"{what}: {tok}")
        assert tok == CRAFT_WANT, what
        assert d_len.cpu().tolist() == [PLEN + 3] * 4 and d_ids[:, PLEN + 2].cpu().tolist() == CRAFT_WANT
        # without the struct: the call it extends (row 0 keeps its seen token, rows 1 and 2 their raw maxima, row 3 the banned 51)
        d_ids = ids.to(DEV)
        d_len = torch.full((4,), PLEN + 2, device=DEV, dtype=torch.int32)
        tok = eng.sample_bias(lg.to(DEV), d_ids, d_len, torch.zeros_like(fin), greedy, None, 0, rows=rows).cpu().tolist()
        assert tok == [7, 41, 51, 51], what
    # a malformed struct is refused on the host
    from genvc_amd._lib import GenvcHipError
    for field, value in (("n_bias", 33), ("reserved", None), ("len", 9), ("ids", V), ("bias", float("nan")), ("bias", float("inf"))):
        bad = logits_bias(CRAFT_KW, PLEN, MAX_NEW, V, EOS)
        if field == "reserved":
            bad.reserved[1] = 1
        elif field == "len":
            bad.len[0] = value
        elif field == "ids":
            bad.ids[1][2] = value
        elif field == "bias":
            bad.bias[0] = value
        else:
            setattr(bad, field, value)
        with pytest.raises(GenvcHipError, match="bias:"):
            eng.sample_bias(lg.to(DEV), ids.to(DEV), torch.full((4,), PLEN + 2, device=DEV, dtype=torch.int32),
                            torch.zeros(4, device=DEV, dtype=torch.int32), greedy, bad, 0)
    eng.close()


# ---- 5. draws -----------------------------------------------------------------------------------------------------------------------
def test_draws_follow_hf():
    """tests/test_gpu_processors.py::test_min_p_draws_follow_hf's count (64 rows x 80 steps) and test (chi-square at 1 - 1e-4) on one
    fixed row with a banned continuation and a finite bias on"""
    from genvc_amd.engine import GptEngine, logits_bias, sample_params
    temperature, top_k = 0.8, 50
    gen = torch.Generator().manual_seed(7)
    s = torch.randn(V, generator=gen) * 2.0
    order = torch.argsort(s, descending=True)
    first, second, lifted = int(order[0]), int(order[1]), int(order[60])
    n0 = 8
    row = [1] * (n0 - 2) + [1024, 9]
    # the most likely token is banned behind a 9 (a hit), the second behind a 10 (a miss); one from outside the top 50 is lifted into it
    kw = dict(bad_words_ids=[[9, first], [10, second]], sequence_bias={(lifted,): 3.0, (1024, 9, second): -0.5})
    chain = BI.hf_chain(kw, n0, EOS, 1.0, MAX_NEW, sampling=dict(temperature=temperature, top_k=top_k))
    p_hf = torch.softmax(BI.run_chain(chain, torch.tensor([row]), s[None])[0], -1)
    kept = p_hf > 0
    assert int(kept.sum()) == top_k and not bool(kept[first]) and bool(kept[second]) and bool(kept[lifted])
    B, steps = 64, 80
    eng = GptEngine(gcfg.gpt_dims(TINY), max_slots=4)
    params = sample_params(dict(repetition_penalty=1.0, temperature=temperature, top_p=1.0, top_k=top_k), V, EOS, seed=11)
    bias = logits_bias(kw, n0, MAX_NEW, V, EOS)
    logits = s.to(DEV).expand(B, V).contiguous()
    counts = torch.zeros(V, dtype=torch.long)
    for step in range(steps):
        ids = torch.ones(B, n0 + 2, device=DEV, dtype=torch.int32)
        ids[:, :n0] = torch.tensor(row, dtype=torch.int32)
        ids_len = torch.full((B,), n0, device=DEV, dtype=torch.int32)
        fin = torch.zeros(B, device=DEV, dtype=torch.int32)
        tok = eng.sample_bias(logits, ids, ids_len, fin, params, bias, step)
        counts += torch.bincount(tok.long().cpu(), minlength=V)
    n = B * steps
    assert int(counts[first]) == 0, "a banned continuation was drawn"
    assert int(counts[~kept].sum()) == 0, "a draw outside HF's kept set"
    exp = p_hf.double() * n
    obs = counts.double()
    big = exp >= 5
    stat = float(((obs[big] - exp[big]) ** 2 / exp[big]).sum())
    rest_e, rest_o = float(exp[~big & kept].sum()), float(obs[~big & kept].sum())
    dof = int(big.sum()) - 1
    if rest_e > 0:
        stat += (rest_o - rest_e) ** 2 / rest_e
        dof += 1
    z = 3.719          # Wilson-Hilferty: the chi-square quantile at 1 - 1e-4
    crit = dof * (1 - 2 / (9 * dof) + z * math.sqrt(2 / (9 * dof))) ** 3
    print(f"chi-square {stat:.1f} against {crit:.1f} at {dof} degrees of freedom; the lifted token was drawn {int(counts[lifted])} times")
    assert stat < crit, (stat, crit, dof)
    eng.close()


# ---- 6. generate, greedy, with output_scores and output_logits ------------------------------------------------------------------------
def first_bigram(ids, b):
    """the first bigram of generated tokens in row b of the baseline, neither of them the stop token: (t, (ids[b, t - 1], ids[b, t]))"""
    for t in range(1, ids.shape[1]):
        if ids[b, t - 1] != EOS and ids[b, t] != EOS:
            return t, (int(ids[b, t - 1]), int(ids[b, t]))
    raise AssertionError("the baseline row has no bigram")


def built_from(base, b_ban=0, b_bias=1, t_bias=2):
    """the kwargs of every case, constructed from the unbiased run `base` (ids, margins): the bigram at its first place in row b_ban is
    banned, and the token row b_bias emits at step t_bias is biased down by the row's top-1 / top-2 gap there and 1.0 more.  Both change
    the greedy run for certain."""
    t, bigram = first_bigram(base["ids"], b_ban)
    tok, gap = int(base["ids"][b_bias, t_bias]), float(base["margins"][b_bias, t_bias])
    assert tok != EOS and np.isfinite(gap)
    sb = {(tok,): -(gap + 1.0), (bigram[0], tok): -0.25}
    return dict(sequence_bias=dict(sequence_bias=sb), bad_words_ids=dict(bad_words_ids=[[EOS], list(bigram)]),
                forced_eos=dict(forced_eos_token_id=EOS), renormalize=dict(renormalize_logits=True),
                all=dict(sequence_bias=sb, bad_words_ids=[[EOS], list(bigram)], forced_eos_token_id=EOS, renormalize_logits=True,
                         forced_bos_token_id=3, min_new_tokens=2, suppress_tokens=[int(base["ids"][b_ban, 0])])), (t, bigram, tok)


def has_bigram(ids, bigram):
    ids = np.asarray(ids)
    return bool(((ids[:, :-1] == bigram[0]) & (ids[:, 1:] == bigram[1])).any())


@pytest.mark.parametrize("rep", [1.0, 2.0])
@pytest.mark.parametrize("case", ["sequence_bias", "bad_words_ids", "forced_eos", "renormalize", "all"])
def test_greedy_generate_against_the_oracle(case, rep):
    seed = 0
    base = TS.plain(TINY, seed, rep)
    kws, (t_ban, bigram, tok) = built_from(base)
    kw = kws[case]
    ora = TS.oracle_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    g = TG.make_gpt(TINY, seed)
    gkw = dict(do_sample=False, repetition_penalty=rep, **kw)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **gkw)
    lat = g.last_latents.clone()
    out = g.generate(cond.to(DEV), codes.to(DEV), **gkw, **BOTH)
    assert torch.equal(out.sequences, bare) and torch.equal(out.latents, lat)
    ids = bare.cpu()
    print(f"{case}, rep {rep}: baseline {base['ids'].tolist()} -> {ids.tolist()}")
    if case == "renormalize":
        assert np.array_equal(ids.numpy(), base["ids"]) or not TS.screened(base, rep)       # the tokens do not move (item 8 holds them bit for bit)
    else:
        assert ids.shape != base["ids"].shape or not np.array_equal(ids.numpy(), base["ids"])   # the case fires
    if case in ("bad_words_ids", "all"):
        assert not has_bigram(ids.numpy(), bigram) and has_bigram(base["ids"], bigram)
    if case in ("forced_eos", "all"):
        assert ids.shape[1] == MAX_NEW and bool((ids[:, -1] == EOS).all())
    # every step against the oracle teacher-forced with the device's tokens; no case is dropped
    r = BI.decode(ora, cond, codes, rep=rep, kw=kw, max_new=MAX_NEW, forced=ids)
    TS.check_tokens(ids, r, rep * 2e-3)
    n = ids.shape[1]
    assert len(out.scores) == n and len(out.logits) == n
    compare(stacked(out.logits), want(r["logits"]), TOL, "logits")
    compare(stacked(out.scores), want(r["scores"]), TOL * max(rep, 1.0), "scores")
    # where the oracle's own margins pass the screen, its free-running ids too
    free = BI.decode(ora, cond, codes, rep=rep, kw=kw, max_new=MAX_NEW)
    if TS.screened(free, rep):
        assert np.array_equal(ids.numpy(), free["ids"])
    if case == "all":
        # a generation split into calls (5 + 5 + 2 steps) restages the struct and stores the same rows
        split = g.generate(cond.to(DEV), codes.to(DEV), group=5, **gkw, **BOTH)
        assert torch.equal(split.sequences, bare) and torch.equal(stacked(split.scores), stacked(out.scores))
    TG.close(g)


def test_one_stream_with_every_kwarg():
    """B = 1: the deferred one-stream loop (decode variant 3) carries the struct as the rows loop does"""
    seed, rep = 0, 1.0
    base = TS.plain(TINY, seed, rep, b=1)
    kws, (_, bigram, _) = built_from(base, b_ban=0, b_bias=0, t_bias=4)
    kw = kws["all"]
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY), None, 1)[:2]
    g = TG.make_gpt(TINY, seed)
    gkw = dict(do_sample=False, repetition_penalty=rep, **kw)
    out = g.generate(cond.to(DEV), codes.to(DEV), **gkw, **BOTH)
    assert g.engine.decode_variant() == 3
    ids = out.sequences.cpu()
    assert not np.array_equal(ids.numpy(), base["ids"]) and not has_bigram(ids.numpy(), bigram) and int(ids[0, -1]) == EOS
    r = BI.decode(TS.oracle_gpt(TINY, seed), cond, codes, rep=rep, kw=kw, max_new=MAX_NEW, forced=ids)
    TS.check_tokens(ids, r, rep * 2e-3)
    compare(stacked(out.scores), want(r["scores"]), TOL, "scores")
    compare(stacked(out.logits), want(r["logits"]), TOL, "logits")
    assert torch.equal(g.generate(cond.to(DEV), codes.to(DEV), **gkw), out.sequences)
    TG.close(g)


# ---- 7. forced EOS --------------------------------------------------------------------------------------------------------------------
FORCE_STOP_BIAS = 2.5          # tests/test_gpu_scores.py: at 2.5 row 1 of a B = 3 call stops at step 1, rows 0 and 2 run all 12 steps
FORCE_SAMPLING = dict(do_sample=True, top_k=8, temperature=0.8, seed=5)


@pytest.mark.parametrize("sampling", [False, True], ids=["greedy", "sampling"])
def test_forced_eos_ends_the_live_rows(sampling):
    seed = 0
    r = TS.plain(TINY, seed, 1.0, stop_bias=FORCE_STOP_BIAS, b=3)
    live_ref = ~(r["ids"][:, :-1] == EOS).any(1)
    assert r["ids"].shape[1] == MAX_NEW and live_ref.any() and not live_ref.all()      # a row is live at the last step, another is not
    g = TG.make_gpt(TINY, seed, stop_bias=FORCE_STOP_BIAS)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY), None, 3)[:2]
    kw = dict(FORCE_SAMPLING) if sampling else dict(do_sample=False)
    kw["repetition_penalty"] = 1.0
    off = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    on = g.generate(cond.to(DEV), codes.to(DEV), forced_eos_token_id=EOS, **kw, **BOTH)
    a, b = off.sequences.cpu(), on.sequences.cpu()
    print(f"without {a.tolist()}\nwith    {b.tolist()}")
    assert a.shape[1] == MAX_NEW and b.shape[1] == MAX_NEW
    live = ~(a[:, :-1] == EOS).any(1)
    assert bool(live.any()), "no row of the device's run is live at the last step"
    if not sampling:
        assert np.array_equal(a.numpy(), r["ids"])
    assert bool((b[:, -1] == EOS).all()) and bool((a[live, -1] != EOS).any())            # the forced step changes a live row's token
    last = stacked(on.scores)[:, -1]
    expect = torch.full((3, V), NINF)
    expect[:, EOS] = 0.0
    assert torch.equal(last, expect)
    # earlier steps: the call without the kwarg, bit for bit
    assert torch.equal(a[:, :-1], b[:, :-1])
    assert torch.equal(stacked(on.scores)[:, :-1], stacked(off.scores)[:, :-1]) and torch.equal(stacked(on.logits), stacked(off.logits))
    assert torch.equal(on.latents, off.latents)
    TG.close(g)


# ---- 8. renormalize_logits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,rep", [(dict(do_sample=False), 2.0), (dict(do_sample=True, top_k=15, temperature=0.75, seed=5), 1.0),
                                    (dict(do_sample=True, top_k=1, temperature=0.75), 1.0)], ids=["greedy", "sampling", "top_k_1"])
def test_renormalized_scores(kw, rep):
    seed = 0
    g = TG.make_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    kw = dict(kw, repetition_penalty=rep, suppress_tokens=[3, 700])
    off = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    on = g.generate(cond.to(DEV), codes.to(DEV), renormalize_logits=True, **kw, **BOTH)
    assert torch.equal(on.sequences, off.sequences) and torch.equal(on.latents, off.latents)
    assert torch.equal(stacked(on.logits), stacked(off.logits))
    got, raw = stacked(on.scores), stacked(off.scores)
    assert bool(torch.isinf(raw).any()) and torch.equal(torch.isinf(got), torch.isinf(raw)) and not bool(torch.isnan(got).any())
    lse = torch.logsumexp(got.double(), -1)
    print(f"largest |logsumexp| {float(lse.abs().max()):.3e} (1e-5); finite entries per row {int(torch.isfinite(got).sum(-1).min())}.."
          f"{int(torch.isfinite(got).sum(-1).max())}")
    assert float(lse.abs().max()) <= 1e-5
    temp = kw.get("temperature", 1.0) if kw["do_sample"] else 1.0
    compare(got, torch.log_softmax(raw, -1), TOL * max(rep, 1.0) / temp, "log_softmax of the stored rows")
    # without output_scores the kwarg changes nothing
    assert torch.equal(g.generate(cond.to(DEV), codes.to(DEV), renormalize_logits=True, **kw), off.sequences)
    TG.close(g)


# ---- 9. guidance ----------------------------------------------------------------------------------------------------------------------
def test_sequence_bias_acts_on_the_guided_row():
    scale, rep, seed = 1.5, 1.0, 0
    base = TG.oracle(TINY, seed, scale, rep)
    TG.screen(base, scale, rep)
    tok, gap = int(base["ids"][0, 2]), float(base["margins"][0, 2])
    assert tok != EOS
    kw = dict(sequence_bias={(tok,): -(gap + 1.0)}, bad_words_ids=[[int(base["ids"][1, 0]), int(base["ids"][1, 1])]])
    g = TG.make_gpt(TINY, seed)
    cond, codes, ncond, ncodes = TG.inputs(gcfg.gpt_dims(TINY))
    gkw = TG.greedy_kw(scale, rep, ncond, ncodes, **kw)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **gkw)
    out = g.generate(cond.to(DEV), codes.to(DEV), **gkw, **BOTH)
    ids = bare.cpu()
    assert torch.equal(out.sequences, bare) and not np.array_equal(ids.numpy(), base["ids"])
    r = BI.decode(base["ora"], cond, codes, rep=rep, kw=kw, max_new=MAX_NEW, forced=ids, guide=(ncond, ncodes, scale))
    TS.check_tokens(ids, r, rep * (2 * scale - 1) * 2e-3)
    compare(stacked(out.scores), want(r["scores"]), TOL * (2 * scale - 1), "guided scores")
    compare(stacked(out.logits), want(r["logits"]), TOL, "conditional logits")
    TG.close(g)


# ---- 10. num_return_sequences ---------------------------------------------------------------------------------------------------------
NRS_SEED = 5


def oracle_draws(ora, cond, codes, kw, seed, sampling, max_new=MAX_NEW):
    """the sampling loop on the oracle: the executed chain, then the oracle's own inverse-CDF draw keyed (seed, step, row)"""
    O = BI.CF.O
    eos = ora.dims["stop_audio_token"]
    fake, logits, cache = ora.prefill(cond, codes)
    chain = BI.hf_chain(kw, fake.shape[1], eos, 1.0, max_new, sampling)
    ids = fake.long()
    fin = torch.zeros(ids.shape[0], dtype=torch.bool)
    toks = []
    for t in range(max_new):
        x = O.sample_from_scores(BI.run_chain(chain, ids, logits), seed, t)
        x[fin] = eos
        toks.append(x)
        ids = torch.cat([ids, x[:, None]], 1)
        fin = fin | (x == eos)
        if bool(fin.all()) or t == max_new - 1:
            break
        logits, cache = ora.step(cache, x, t + 1)
    return torch.stack(toks, 1).numpy()


def test_num_return_sequences_never_holds_the_banned_bigram():
    seed, N = 0, 2
    sampling = dict(temperature=0.75, top_k=15)
    ora = TS.oracle_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    c2, k2 = cond.repeat_interleave(N, 0), codes.repeat_interleave(N, 0)
    free = oracle_draws(ora, c2, k2, {}, NRS_SEED, sampling)
    _, bigram = first_bigram(free, 0)
    kw = dict(bad_words_ids=[list(bigram)])
    ref = oracle_draws(ora, c2, k2, kw, NRS_SEED, sampling)
    # the seed is picked so that on the oracle the ban fires and its prefix token is still drawn
    assert has_bigram(free, bigram) and not has_bigram(ref, bigram) and bool((ref == bigram[0]).any())
    g = TG.make_gpt(TINY, seed)
    gkw = dict(do_sample=True, repetition_penalty=1.0, seed=NRS_SEED, num_return_sequences=N, **sampling)
    plain = g.generate(cond.to(DEV), codes.to(DEV), **gkw).cpu().numpy()
    got = g.generate(cond.to(DEV), codes.to(DEV), **gkw, **kw).cpu().numpy()
    print(f"bigram {bigram}\nwithout {plain.tolist()}\nwith    {got.tolist()}\noracle  {ref.tolist()}")
    assert got.shape[0] == TG.B * N and has_bigram(plain, bigram)
    assert not has_bigram(got, bigram), "a returned row contains the banned bigram"
    assert bool((got == bigram[0]).any()), "the prefix token of the banned bigram does not occur"
    TG.close(g)


# ---- 11. off is off -------------------------------------------------------------------------------------------------------------------
OFF = dict(sequence_bias={}, bad_words_ids=[[EOS]], forced_eos_token_id=None, forced_bos_token_id=3, renormalize_logits=False)


@pytest.mark.parametrize("kw", [dict(do_sample=False, repetition_penalty=2.0), dict(do_sample=True, top_k=15, temperature=0.75, seed=5)],
                         ids=["greedy", "sampling"])
def test_off_is_off(kw, monkeypatch):
    g = TG.make_gpt(TINY, 0)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    calls = []
    real = g.engine.generate_bias
    monkeypatch.setattr(g.engine, "generate_bias", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    a = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    la = g.last_latents.clone()
    for off in (OFF, dict(sequence_bias=None, bad_words_ids=[], renormalize_logits=None), dict(sequence_bias=[])):
        b = g.generate(cond.to(DEV), codes.to(DEV), **kw, **off)
        assert torch.equal(a, b) and torch.equal(la, g.last_latents)
        o = g.generate(cond.to(DEV), codes.to(DEV), **kw, **off, **BOTH)
        assert torch.equal(o.sequences, a)
    assert not calls
    g.generate(cond.to(DEV), codes.to(DEV), **kw, renormalize_logits=True)
    assert len(calls) == 1          # (the wrapper does count)
    TG.close(g)
