"""GPU: per-step scores and logits of GPT.generate (return_dict_in_generate / output_scores / output_logits; include/genvc_hip.h:
gvc_gpt_generate_scores, gvc_transition_scores) against tests/scores_oracle.py and tests/cfg_oracle.py -- the oracle's GPT forward
followed by the installed transformers' own processor and warper objects, executed.  Tolerances: the project's 1e-4 logit tolerance,
times what the chain does to an error of the logits (the repetition penalty's factor, 1 / temperature, 2s - 1 for the guidance
combine).  Greedy cases are margin-screened on the oracle as tests/test_gpu_cfg.py screens them and assert the screen; the one case
the issue names that misses it on the oracle (model seed 0 at rep 2) is written up in test_greedy_scores_and_logits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_oracle as CF                       # noqa: E402
import scores_oracle as SO                    # noqa: E402
import test_gpu_cfg as TG                     # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = TG.EOS, TG.V
MAX_NEW = TG.MAX_NEW          # 12
TINY = gcfg.TINY_MODEL_ARGS
TOL = 1e-4                    # the project's logit tolerance
BOTH = dict(return_dict_in_generate=True, output_scores=True, output_logits=True)
FULL2_SEED = 0                # model seed of the full-width case, picked by the CPU screen: margin 1.4e-2 against 2e-3 (seed 3: 6.6e-4)

_ora, _plain = {}, {}


def oracle_gpt(model_args, seed, stop_bias=None):
    """the oracle's model for these weights, built once per session"""
    key = (id(model_args), seed, stop_bias)
    if key not in _ora:
        dims = gcfg.gpt_dims(model_args)
        w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
        if stop_bias is not None:
            w["mel_head.bias"][EOS] = float(stop_bias)
        _ora[key] = CF.BO.OracleGpt(w, dims)
    return _ora[key]


def plain(model_args, seed, rep, kw=None, stop_bias=None, b=TG.B):
    """the CPU restatement of one unguided greedy case, computed once per session and shared (read-only)"""
    key = (id(model_args), seed, rep, repr(sorted((kw or {}).items())), stop_bias, b)
    if key not in _plain:
        cond, codes = TG.inputs(gcfg.gpt_dims(model_args), None, b)[:2]
        _plain[key] = SO.decode(oracle_gpt(model_args, seed, stop_bias), cond, codes, rep=rep, kw=kw, max_new=MAX_NEW)
    return _plain[key]


def stacked(rows):
    """a tuple of n [R, V] device rows -> [R, n, V] on the CPU"""
    return torch.stack(tuple(rows), 1).cpu()


def want(rows):
    return torch.stack(list(rows), 1)


def compare(got, ref, tol, what):
    """got / ref [R, n, V]: the -inf pattern equal exactly, every other entry within tol; prints the figure before it asserts"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    gi, ri = torch.isinf(got) & (got < 0), torch.isinf(ref) & (ref < 0)
    same = bool((gi == ri).all())
    live = ~(gi | ri)
    err = float((got - ref)[live].abs().max()) if bool(live.any()) else 0.0
    print(f"{what}: max abs err {err:.3e} (tolerance {tol:.1e}), -inf entries {int(ri.sum())}, pattern equal {same}")
    assert same, f"{what}: the -inf pattern differs in {int((gi != ri).sum())} entries"
    assert bool(torch.isfinite(got[live]).all()) and err <= tol, f"{what}: {err:.3e} > {tol:.1e}"


def screened(r, rep):
    """tests/test_gpu_cfg.py's screen on the oracle's own margins, without guidance: 2e-3 times the repetition penalty's factor"""
    m = r["margins"]
    floor, need = float(m[np.isfinite(m)].min()), rep * 2e-3
    print(f"oracle margin {floor:.3e} (screen {need:.1e}): {'screened' if floor >= need else 'NOT screened'}")
    return floor >= need


def check_tokens(ids, ref, need):
    """the device's tokens against the oracle teacher-forced with them: while a row is live, its token's oracle score lies within `need`
    (the screen) of the row's maximum -- so it IS the oracle's argmax wherever the oracle's margin exceeds the screen"""
    sc = want(ref["scores"])
    gap = sc.max(-1)[0] - sc.gather(2, ids[:, :, None]).squeeze(2)
    live = torch.ones_like(ids, dtype=torch.bool)
    live[:, 1:] = (ids[:, :-1] != EOS).cumprod(1).bool()
    print(f"largest (oracle maximum - oracle score of the device's token) {float(gap[live].max()):.3e} (screen {need:.1e})")
    assert bool((gap[live] <= need).all())
    assert bool((ids[~live] == EOS).all())


# ---- 1. greedy ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1.0, 2.0])
@pytest.mark.parametrize("seed", [0, 3])
def test_greedy_scores_and_logits(seed, rep):
    """Model seeds 0 and 3 at rep 1 and 2, input seed 13.  Screened on the CPU: (0, 1) 2.1e-2, (3, 1) and (3, 2) 1.1e-2 pass; (0, 2)
    does NOT -- its smallest margin is 1.37e-3 (row 0, step 5, two unseen tokens with raw logits 2.07268 / 2.07132) against a screen of
    4e-3, and below the plain 2e-3 too.  So a case that passes the screen asserts the oracle's greedy ids; every case, screened or
    not, is then compared step by step against the oracle teacher-forced with the device's tokens -- logits, scores, and each token
    within the screen of the oracle's maximum (check_tokens), which is the id comparison wherever the margin carries it."""
    r = plain(TINY, seed, rep)
    ok = screened(r, rep)
    g = TG.make_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    kw = dict(do_sample=False, repetition_penalty=rep)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    lat = g.last_latents.clone()
    out = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    assert torch.equal(out.sequences, bare) and torch.equal(out.latents, lat)
    if ok:
        assert np.array_equal(bare.cpu().numpy(), r["ids"])
    else:
        r = SO.decode(oracle_gpt(TINY, seed), cond, codes, rep=rep, forced=bare.cpu())
    check_tokens(bare.cpu(), r, rep * 2e-3)
    n = out.sequences.shape[1]
    assert len(out.scores) == n and len(out.logits) == n and tuple(out.scores[0].shape) == (TG.B, V)
    compare(stacked(out.logits), want(r["logits"]), TOL, "logits")
    compare(stacked(out.scores), want(r["scores"]), TOL * max(rep, 1.0), "scores")
    # only what was asked for is there
    one = g.generate(cond.to(DEV), codes.to(DEV), **kw, return_dict_in_generate=True, output_logits=True)
    assert one.scores is None and torch.equal(stacked(one.logits), stacked(out.logits)) and torch.equal(one.sequences, bare)
    if seed == 0 and rep == 2.0:
        # greedy search has no Temperature in HF: the stored row does not move with the kwarg (the device sampler divides by it)
        t = g.generate(cond.to(DEV), codes.to(DEV), temperature=0.6, **kw, **BOTH)
        assert torch.equal(t.sequences, g.generate(cond.to(DEV), codes.to(DEV), temperature=0.6, **kw)) and torch.equal(t.sequences, bare)
        assert torch.equal(stacked(t.scores), stacked(out.scores)) and torch.equal(stacked(t.logits), stacked(out.logits))
    if seed == 0 and rep == 1.0:
        # sampling with top_k = 1: Temperature, then TopK at k = 1 leaves the maximum alone, at its temperature-scaled score
        temp = 0.75
        s1 = g.generate(cond.to(DEV), codes.to(DEV), do_sample=True, top_k=1, temperature=temp, repetition_penalty=rep, **BOTH)
        assert torch.equal(s1.sequences, bare)
        ref = SO.decode(oracle_gpt(TINY, seed), cond, codes, rep=rep, sampling=dict(temperature=temp, top_k=1), forced=bare.cpu())
        compare(stacked(s1.scores), want(ref["scores"]), TOL / temp, "scores at top_k = 1")
        assert int(torch.isfinite(stacked(s1.scores)).sum()) == TG.B * n
    TG.close(g)


# ---- 2. processors --------------------------------------------------------------------------------------------------------------------
def test_processor_bans_show_in_the_scores():
    """tests/test_gpu_cfg.py's PROC_CASE settings without guidance: the stop token held off by min_new_tokens = 6 (and whatever
    no_repeat_ngram_size = 2 bans: nothing in this case, no token repeats) are -inf entries of the scores, the same ones as the oracle's
    at every step (integer logic: compare() asserts the pattern exactly).  A second call adds suppress_tokens, so that entries other
    than the stop token are banned too."""
    c = TG.PROC_CASE
    g = TG.make_gpt(TINY, c["seed"], stop_bias=c["stop_bias"])
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    kw = dict(do_sample=False, repetition_penalty=c["rep"], **c["kw"])
    bare = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    out = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    assert torch.equal(out.sequences, bare)
    # the bans depend on the ids alone, so the oracle is teacher-forced with the device's tokens (the greedy margins of this model seed
    # at rep 2 miss the screen: test_greedy_scores_and_logits), and the tokens are held to the screen's width of its maximum
    r = SO.decode(oracle_gpt(TINY, c["seed"], c["stop_bias"]), cond, codes, rep=c["rep"], kw=c["kw"], forced=bare.cpu())
    check_tokens(bare.cpu(), r, c["rep"] * 2e-3)
    ref = want(r["scores"])
    assert ref.shape[1] > 6 and bool(torch.isinf(ref[:, :6, EOS]).all()) and not bool(torch.isinf(ref[:, 6:, EOS]).any())  # min_new_tokens
    compare(stacked(out.scores), ref, TOL * c["rep"], "scores")
    compare(stacked(out.logits), want(r["logits"]), TOL, "logits")
    assert not bool(torch.isinf(stacked(out.logits)).any())
    kw2 = dict(kw, suppress_tokens=[3, 700, 1024])
    bare2 = g.generate(cond.to(DEV), codes.to(DEV), **kw2)
    out2 = g.generate(cond.to(DEV), codes.to(DEV), **kw2, **BOTH)
    assert torch.equal(out2.sequences, bare2)
    r2 = SO.decode(oracle_gpt(TINY, c["seed"], c["stop_bias"]), cond, codes, rep=c["rep"], kw=dict(c["kw"], suppress_tokens=[3, 700, 1024]),
                   forced=bare2.cpu())
    check_tokens(bare2.cpu(), r2, c["rep"] * 2e-3)
    assert bool(torch.isinf(want(r2["scores"])[:, :, [3, 700, 1024]]).all())
    compare(stacked(out2.scores), want(r2["scores"]), TOL * c["rep"], "scores with suppress_tokens")
    TG.close(g)


# ---- 3. sampling ----------------------------------------------------------------------------------------------------------------------
TOP_K, TEMP = 15, 0.75


def check_top_k_rows(got, full, what):
    """got [R, n, V]: the device's scores of a top_k = 15 draw; full [R, n, V]: the oracle's temperature-scaled rows before TopK,
    teacher-forced with the device's tokens.  Around the oracle's 15th score lies a band of +-delta, the project's 2e-3 logit screen
    behind the temperature: above it an entry must be kept, at its score; below it it must be -inf; inside it either.  -> the number of
    in-band entries other than the 15th itself, for the caller's bound"""
    delta = 2e-3 / TEMP
    kth = torch.topk(full, TOP_K, dim=-1)[0][..., -1:]
    above, below = full > kth + delta, full < kth - delta
    finite = torch.isfinite(got)
    err = float((got - full)[above & finite].abs().max())
    in_band = int((~above & ~below).sum()) - full.shape[0] * full.shape[1]
    print(f"{what}: max abs err above the band {err:.3e} (tolerance {TOL / TEMP:.1e}); in-band entries besides the 15th: {in_band} over "
          f"{full.shape[0] * full.shape[1]} row-steps; finite per row-step {int(finite.sum(-1).min())}..{int(finite.sum(-1).max())}")
    assert bool(finite[above].all()), f"{what}: {int((above & ~finite).sum())} entries above the band were dropped"
    assert err <= TOL / TEMP
    assert bool((torch.isinf(got) & (got < 0))[below].all()), f"{what}: {int((below & finite).sum())} entries below the band were kept"
    assert not bool(torch.isnan(got).any()) and int(finite.sum(-1).min()) >= TOP_K
    return in_band


@pytest.mark.parametrize("seed", [0, 3])
def test_sampling_scores_hold_the_top_k(seed):
    g = TG.make_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    kw = dict(do_sample=True, top_k=TOP_K, temperature=TEMP, repetition_penalty=1.0, seed=5)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    out = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    assert torch.equal(out.sequences, bare)
    ref = SO.decode(oracle_gpt(TINY, seed), cond, codes, sampling=dict(temperature=TEMP, top_k=0), forced=bare.cpu())
    compare(stacked(out.logits), want(ref["logits"]), TOL, "logits")
    rows = TG.B * bare.shape[1]
    in_band = check_top_k_rows(stacked(out.scores), want(ref["scores"]), "scores")
    # measured on the oracle alone: the 16th score lies inside the band in about a tenth of the row-steps.  Above one per row-step the
    # band would decide nothing
    assert in_band <= rows, f"{in_band} in-band entries over {rows} row-steps"
    # every drawn token is one the scores kept
    picked = stacked(out.scores).gather(2, bare.cpu()[:, :, None]).squeeze(2)
    live = torch.ones_like(bare.cpu(), dtype=torch.bool)
    live[:, 1:] = (bare.cpu()[:, :-1] != EOS).cumprod(1).bool()
    assert bool(torch.isfinite(picked[live]).all())
    TG.close(g)


# ---- 4. guided ------------------------------------------------------------------------------------------------------------------------
def test_guided_scores_and_conditional_logits():
    scale, rep, seed = 1.5, 1.0, 0
    r = TG.oracle(TINY, seed, scale, rep)
    TG.screen(r, scale, rep)
    g = TG.make_gpt(TINY, seed)
    cond, codes, ncond, ncodes = TG.inputs(gcfg.gpt_dims(TINY))
    kw = TG.greedy_kw(scale, rep, ncond, ncodes)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    out = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    assert torch.equal(out.sequences, bare) and np.array_equal(bare.cpu().numpy(), r["ids"])
    compare(stacked(out.scores), want(r["scores"]), TOL * (2 * scale - 1), "guided scores")
    # the logits are the conditional rows, as in HF: the model under the conditional prompt, fed the guided tokens
    ref = SO.decode(r["ora"], cond, codes, forced=torch.from_numpy(r["ids"]))
    compare(stacked(out.logits), want(ref["logits"]), TOL, "conditional logits")
    TG.close(g)


# ---- 5. items under different scales, and rows that outlive one another ---------------------------------------------------------------
SCALES = (1.5, None, 3.0)
SCREENS = (4e-3, 2e-3, 1e-2)          # 2e-3 * (2s - 1)


def one_item(ora, i, scale, cond, codes, ncond, ncodes):
    if scale is None:
        return SO.decode(ora, cond[i:i + 1], codes[i:i + 1], max_new=MAX_NEW)
    return CF.guided(ora, cond[i:i + 1], codes[i:i + 1], ncond[i:i + 1], ncodes[i:i + 1], scale, max_new=MAX_NEW)


@pytest.mark.parametrize("stop_bias", [None, 3.0])
def test_items_decoded_alone_under_their_own_scale(stop_bias):
    """three items of input seed 13, item i decoded alone under SCALES[i]; with the stop bias they stop at different steps"""
    seed = 0
    ora = oracle_gpt(TINY, seed, stop_bias)
    cond, codes, ncond, ncodes = TG.inputs(gcfg.gpt_dims(TINY), None, 3)
    g = TG.make_gpt(TINY, seed, stop_bias=stop_bias)
    lens = []
    for i, scale in enumerate(SCALES):
        r = one_item(ora, i, scale, cond, codes, ncond, ncodes)
        TG.screen(r, 1.0 if scale is None else scale, 1.0)
        kw = dict(do_sample=False, repetition_penalty=1.0) if scale is None else TG.greedy_kw(scale, 1.0, ncond[i:i + 1], ncodes[i:i + 1])
        bare = g.generate(cond[i:i + 1].to(DEV), codes[i:i + 1].to(DEV), **kw)
        out = g.generate(cond[i:i + 1].to(DEV), codes[i:i + 1].to(DEV), **kw, **BOTH)
        assert torch.equal(out.sequences, bare) and np.array_equal(bare.cpu().numpy(), r["ids"])
        compare(stacked(out.scores), want(r["scores"]), TOL * (1.0 if scale is None else 2 * scale - 1), f"item {i} (scale {scale}) scores")
        lens.append(bare.shape[1])
    print(f"lengths {lens}")
    if stop_bias is not None:
        assert len(set(lens)) > 1 and min(lens) == 1
    TG.close(g)


@pytest.mark.parametrize("stop_bias", [3.0, 2.5])
def test_stopped_rows_keep_matching_the_oracle(stop_bias):
    """one unguided B = 3 call with a stop bias: the rows that have stopped are fed the stop token and keep storing rows -- the
    oracle's, which is fed the same.  At 3.0 all three rows of the UNGUIDED call stop at step 0 on the oracle (the steps 0, 0 and 4 are
    those of the items under their scales, above), so no row outlives another; at 2.5 row 1 stops at step 1 and rows 0 and 2 run the
    whole 12 steps beside it (oracle margin 2.1e-2)."""
    seed = 0
    r = plain(TINY, seed, 1.0, stop_bias=stop_bias, b=3)
    TG.screen(r, 1.0, 1.0)
    stops = [int(np.nonzero(row == EOS)[0][0]) if (row == EOS).any() else MAX_NEW for row in r["ids"]]
    print(f"oracle stop steps {stops}")
    if stop_bias == 2.5:
        assert len(set(stops)) > 1 and min(stops) < r["ids"].shape[1] - 2          # a row outlives another by many steps
    g = TG.make_gpt(TINY, seed, stop_bias=stop_bias)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY), None, 3)[:2]
    kw = dict(do_sample=False, repetition_penalty=1.0)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    out = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    assert torch.equal(out.sequences, bare) and np.array_equal(bare.cpu().numpy(), r["ids"])
    compare(stacked(out.scores), want(r["scores"]), TOL, "scores, stopped rows included")
    compare(stacked(out.logits), want(r["logits"]), TOL, "logits, stopped rows included")
    TG.close(g)


# ---- 6. num_return_sequences ----------------------------------------------------------------------------------------------------------
def test_num_return_sequences_rows():
    seed, N = 0, 3
    g = TG.make_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    kw = dict(do_sample=True, top_k=TOP_K, temperature=TEMP, repetition_penalty=1.0, seed=5, num_return_sequences=N)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    out = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    n = bare.shape[1]
    assert torch.equal(out.sequences, bare) and tuple(bare.shape) == (TG.B * N, n)
    assert len(out.scores) == n and tuple(out.scores[0].shape) == (TG.B * N, V) and tuple(out.logits[0].shape) == (TG.B * N, V)
    # row b * N + j is candidate j of item b: the oracle decodes item b's prompt under that row's tokens
    ref = SO.decode(oracle_gpt(TINY, seed), cond.repeat_interleave(N, 0), codes.repeat_interleave(N, 0),
                    sampling=dict(temperature=TEMP, top_k=0), forced=bare.cpu())
    compare(stacked(out.logits), want(ref["logits"]), TOL, "logits")
    in_band = check_top_k_rows(stacked(out.scores), want(ref["scores"]), "scores")
    assert in_band <= TG.B * N * n
    assert len({tuple(row.tolist()) for row in bare.cpu()}) > TG.B          # the candidates of an item differ
    TG.close(g)


def test_keyed_call_mixing_greedy_and_sampled_rows():
    """the engine call with per-row settings (gvc_row_sampling): row 0 has top_k = 1, row 1 top_k = 15, so both run the sampling kernel
    and row 0 takes its top_k == 1 branch, which GPT.generate alone never reaches.  With do_sample the row holds TopK's row at k = 1
    behind the temperature, without it the full row before the temperature; row 1 is a top-15 draw either way"""
    seed = 0
    g = TG.make_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    keys = [dict(repetition_penalty=1.0, temperature=TEMP, top_p=1.0, top_k=k, seed=5, rng_row=r, rng_step0=0) for r, k in enumerate((1, TOP_K))]
    got = {}
    for do_sample in (True, False):
        st = g._start(g.compute_embeddings(cond.to(DEV), codes.to(DEV)), dict(top_k=TOP_K, temperature=TEMP))
        g._step_outputs(st, BOTH)
        g.engine.generate_scores(st["slots"], None, 1.0, st["ids"], st["ids_len"], st["finished"], st["params"], None, 0, MAX_NEW, st["toks"],
                                 st["lats"], scores_out=st["scores"], logits_out=st["raw_logits"], do_sample=do_sample,
                                 max_keys=st["n0"] + MAX_NEW, rows=keys)
        got[do_sample] = (st["toks"].long().cpu(), st["scores"].cpu(), st["raw_logits"].cpu())
    toks = got[True][0]
    assert torch.equal(got[False][0], toks) and torch.equal(got[False][2], got[True][2])          # the flag moves the scores alone
    ora = oracle_gpt(TINY, seed)
    full = SO.decode(ora, cond, codes, sampling=dict(temperature=TEMP, top_k=0), forced=toks)        # temperature-scaled rows, no TopK
    bare = SO.decode(ora, cond, codes, forced=toks)                                                  # no temperature
    compare(got[True][2], want(full["logits"]), TOL, "logits")
    top1 = SO.decode(ora, cond[:1], codes[:1], sampling=dict(temperature=TEMP, top_k=1), forced=toks[:1])
    compare(got[True][1][:1], want(top1["scores"]), TOL / TEMP, "row 0, do_sample: TopK at k = 1")
    compare(got[False][1][:1], want(bare["scores"])[:1], TOL, "row 0, greedy: the full row before the temperature")
    for flag in (True, False):
        assert check_top_k_rows(got[flag][1][1:], want(full["scores"])[1:], f"row 1 (do_sample={flag})") <= MAX_NEW
    check_tokens(toks[:1], dict(scores=[x[:1] for x in bare["scores"]]), 2e-3)                       # row 0 decodes greedily
    TG.close(g)


# ---- 7. one stream --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defer,persist", [("1", "1"), ("0", "1"), ("1", "0")], ids=["deferred", "eager", "launch_per_phase"])
def test_one_stream(defer, persist, monkeypatch):
    monkeypatch.setenv("GVC_DEFER_DECODE", defer)
    monkeypatch.setenv("GVC_PERSIST", persist)
    seed, rep = 0, 1.0
    r = plain(TINY, seed, rep, b=1)
    TG.screen(r, 1.0, rep)
    g = TG.make_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY), None, 1)[:2]
    kw = dict(do_sample=False, repetition_penalty=rep)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    assert (g.engine.decode_variant() == 3) == (persist == "1")
    out = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    assert torch.equal(out.sequences, bare) and np.array_equal(bare.cpu().numpy(), r["ids"])
    compare(stacked(out.scores), want(r["scores"]), TOL, "scores")
    compare(stacked(out.logits), want(r["logits"]), TOL, "logits")
    # a generation split into calls (5 + 5 + 2 steps) stores the same rows at the same steps
    split = g.generate(cond.to(DEV), codes.to(DEV), group=5, **kw, **BOTH)
    assert torch.equal(split.sequences, bare)
    assert torch.equal(stacked(split.scores), stacked(out.scores)) and torch.equal(stacked(split.logits), stacked(out.logits))
    TG.close(g)


# ---- 8. the gather kernel -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 12])
@pytest.mark.parametrize("R", [1, 3])
def test_transition_scores_kernel(R, n):
    from genvc_amd.engine import GptEngine
    eng = GptEngine(gcfg.gpt_dims(TINY), max_slots=2)
    gen = torch.Generator().manual_seed(23 + R + n)
    buf = torch.full((R, 16, V), float("nan"))            # the scores are a column slice of a wider buffer, as generate() hands them out
    toks = torch.zeros(R, n, dtype=torch.long)
    for r in range(R):
        for t in range(n):
            row = (torch.rand(V, generator=gen) * 2 - 1) * 12.0
            drop = (0, 7, 500, V - 15)[(r + t) % 4]       # up to 1011 entries -inf: what a top-15 draw leaves
            row[torch.randperm(V, generator=gen)[:drop]] = -float("inf")
            kept = torch.nonzero(torch.isfinite(row)).squeeze(1)
            toks[r, t] = kept[int(torch.randint(len(kept), (1,), generator=gen))]
            buf[r, t] = row
    dbuf = buf.to(DEV)
    for scores in (dbuf[:, :n], dbuf[:, :n].contiguous()):
        got = eng.transition_scores(scores, toks.to(DEV).int(), normalize=False).cpu()
        assert torch.equal(got, buf[:, :n].gather(2, toks[:, :, None]).squeeze(2))
        got = eng.transition_scores(scores, toks.to(DEV).int(), normalize=True).cpu()
        ref = torch.log_softmax(buf[:, :n], dim=-1).gather(2, toks[:, :, None]).squeeze(2)
        err = float((got - ref).abs().max())
        print(f"R {R} n {n}: log_softmax gather max abs err {err:.3e} (tolerance {TOL:.1e})")
        assert bool(torch.isfinite(got).all()) and err <= TOL
    # a dropped token's score is -inf, one outside the vocabulary NaN
    row = torch.zeros(1, 1, V)
    row[0, 0, 3] = -float("inf")
    got = eng.transition_scores(row.to(DEV), torch.tensor([[3]], dtype=torch.int32, device=DEV), normalize=True).cpu()
    assert float(got) == -float("inf")
    got = eng.transition_scores(row.to(DEV), torch.tensor([[V]], dtype=torch.int32, device=DEV), normalize=False).cpu()
    assert bool(torch.isnan(got).all())
    eng.close()


def test_compute_transition_scores_reads_the_call_buffers():
    """GPT.compute_transition_scores on a call's own outputs: the gather of tests/scores_oracle.py (pinned to HF's method on the CPU)"""
    seed = 0
    g = TG.make_gpt(TINY, seed)
    cond, codes = TG.inputs(gcfg.gpt_dims(TINY))[:2]
    out = g.generate(cond.to(DEV), codes.to(DEV), do_sample=True, top_k=TOP_K, temperature=TEMP, seed=5, **BOTH)
    sc = stacked(out.scores)
    raw = g.compute_transition_scores(out.sequences, out.scores).cpu()
    assert torch.equal(raw, SO.gather(sc, out.sequences.cpu(), False))
    norm = g.compute_transition_scores(out.sequences, out.scores, normalize_logits=True).cpu()
    err = float((norm - SO.gather(sc, out.sequences.cpu(), True)).abs().max())
    print(f"normalised transition scores: max abs err {err:.3e}")
    assert err <= TOL and bool((norm <= 0).all())
    # rows that are no views of one buffer (copies) give the same
    assert torch.equal(g.compute_transition_scores(out.sequences, tuple(s.clone() for s in out.scores), normalize_logits=True).cpu(), norm)
    TG.close(g)


# ---- 9. full width --------------------------------------------------------------------------------------------------------------------
def test_full_width_runs_on_the_rows_step():
    """the default widths with two layers (tests/test_gpu_cfg.py: FULL2): two rows decode on the one-launch rows step (variant 5)"""
    rep = 1.0
    r = plain(TG.FULL2, FULL2_SEED, rep)
    TG.screen(r, 1.0, rep)
    g = TG.make_gpt(TG.FULL2, FULL2_SEED)
    cond, codes = TG.inputs(gcfg.gpt_dims(TG.FULL2))[:2]
    kw = dict(do_sample=False, repetition_penalty=rep)
    bare = g.generate(cond.to(DEV), codes.to(DEV), **kw)
    assert g.engine.decode_variant() == 5
    out = g.generate(cond.to(DEV), codes.to(DEV), **kw, **BOTH)
    assert torch.equal(out.sequences, bare) and np.array_equal(bare.cpu().numpy(), r["ids"])
    compare(stacked(out.scores), want(r["scores"]), TOL, "scores")
    compare(stacked(out.logits), want(r["logits"]), TOL, "logits")
    TG.close(g)
