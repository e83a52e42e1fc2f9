"""GPU: speculative sampling for assisted decoding (GPT.generate(assistant_model=..., speculative_sampling=True); include/genvc_hip.h:
gvc_spec_accept_sample, gvc_gpt_generate_assisted_sample) against its CPU restatement (tests/spec_sample_oracle.py).
1. the accept step (warp kernel + accept kernel, no engine) on planted rows: every output array exactly;  2. the distribution of the
   first token of a round through the kernel;  3. whole generations against the oracle chain of a CPU target and a CPU draft on the
   same uniforms, bit for bit, on seeds whose every decision clears the margins;  4. a self-draft accepts everything, split rounds
   change nothing, and the calls around a sampled assisted call return what they return alone.
Every seed is chosen on the CPU (the searches below run before any GPU work and never repeat a GPU run) and the screen is asserted."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spec_sample_oracle as SO               # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026
MAX_NEW = 12
MARGIN = 1e-4          # the project's draw screen
LOGIT_SCREEN = 2e-3    # the project's logit screen (the GPU's logits are within 1e-4 of the oracle's)
IN_SEED = 13
TC = 6
TINY = gcfg.TINY_MODEL_ARGS
TINY4 = dict(gcfg.TINY_MODEL_ARGS, gpt_layers=4)
FULL2 = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2)
TOL = 1e-4
STATE = ("ids", "ids_len", "finished", "emitted", "pending", "toks", "lats", "drop_target", "drop_assistant", "rounds", "drafted",
         "accepted")


# ---- 1. the accept step against the oracle ----------------------------------------------------------------------------------------------
B_ACC, K_ACC, N0, D_LAT = 8, 5, 20, 8
WIDTH = 60 + MAX_NEW + 16                                # ids columns: the longest row and its round fit
LENS = [20, 25, 30, 35, 40, 45, 50, 55]                  # ids length of every row (the processors' prompt length is N0)
EMITTED = [3, 1, 5, 2, 4, MAX_NEW - 3, 0, 6]             # row 5: k' = 2 < k
FINISHED = [0, 0, 0, 0, 1, 0, 0, 0]                      # row 4 is finished
STOP_ROW, STOP_AT = 3, 1                                 # row 3: draft d_2 is the stop token, and the target agrees with it
_acc_cases = {}


def accept_case(top_k, top_p, rep, kw_key):
    """the inputs of one accept case and the oracle's outputs, computed once and shared (read-only).  The drafts and their warped rows
    come from the oracle's draft side on the target's logits plus uniform(+-0.5); the seed advances until every decision of the accept
    step (accept tests, residual and bonus draws) clears MARGIN"""
    key = (top_k, top_p, rep, kw_key)
    if key in _acc_cases:
        return _acc_cases[key]
    kw = dict(kw_key)
    samp = dict(repetition_penalty=rep, temperature=0.85, top_k=top_k, top_p=top_p)
    logits = synth.uniform(51, "spec_logits", (B_ACC, K_ACC + 1, V), 2.0).float()
    dlogits = (logits[:, :K_ACC] + synth.uniform(52, "spec_draft", (B_ACC, K_ACC, V), 0.5 / 3 ** 0.5)).float()
    logits[STOP_ROW, STOP_AT, EOS] = 40.0
    dlogits[STOP_ROW, STOP_AT, EOS] = 40.0
    # row 6 drafts from the target's own logits: the rule accepts everything there (p == q)
    dlogits[6] = logits[6, :K_ACC]
    latents = synth.uniform(53, "spec_latents", (B_ACC, K_ACC + 1, D_LAT), 1.0).float()
    hist = synth.integers(54, "spec_ids", (B_ACC, max(LENS)), 1024).numpy().astype(np.int32)
    ids = np.ones((B_ACC, WIDTH), dtype=np.int32)
    for b, n in enumerate(LENS):
        ids[b, :n] = hist[b, :n]
    base = dict(ids=ids, ids_len=np.array(LENS, dtype=np.int32), finished=np.array(FINISHED, dtype=np.int32),
                emitted=np.array(EMITTED, dtype=np.int32), pending=np.full(B_ACC, -1, dtype=np.int32),
                toks=np.full((B_ACC, MAX_NEW), EOS, dtype=np.int32), lats=np.zeros((B_ACC, MAX_NEW, D_LAT), dtype=np.float32),
                drop_target=np.zeros(B_ACC, dtype=np.int32), drop_assistant=np.zeros(B_ACC, dtype=np.int32),
                rounds=np.zeros(B_ACC, dtype=np.int32), drafted=np.zeros(B_ACC, dtype=np.int32),
                accepted=np.zeros(B_ACC, dtype=np.int32), max_new=MAX_NEW)
    for seed in range(300, 400):
        ref = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in base.items()}
        drafts, q, _ = SO.draft(dlogits.numpy(), ids, LENS, EMITTED, FINISHED, K_ACC, samp, seed, EOS, kw, N0)
        out = SO.accept(ref, K_ACC, K_ACC + 1, logits.numpy(), latents.numpy(), drafts, q, samp, seed, EOS, kw, N0)
        if min(out["margins"]) > MARGIN:
            break
    _acc_cases[key] = dict(samp=samp, kw=kw, seed=seed, logits=logits, latents=latents, drafts=drafts, q=q, base=base, ref=ref, out=out)
    return _acc_cases[key]


def make_state(base, k):
    from genvc_amd.engine import AssistedState
    B = len(base["ids_len"])
    st = AssistedState(torch.ones(B, base["ids"].shape[1] - base["max_new"] - 16, dtype=torch.int32, device=DEV), k, base["max_new"], EOS,
                       V, base["lats"].shape[-1])
    assert st.ids.shape[1] == base["ids"].shape[1]
    st.ids.copy_(torch.from_numpy(base["ids"]))
    for n in ("ids_len", "finished", "emitted"):
        getattr(st, n).copy_(torch.from_numpy(base[n]))
    return st


def compare_state(st, ref):
    for name in STATE:
        got = getattr(st, name).cpu().numpy()
        want = ref[name]
        assert np.array_equal(got, want), (name, got, want)


@pytest.mark.parametrize("kw", [(), (("min_new_tokens", 3),), (("no_repeat_ngram_size", 2),), (("min_p", 0.05),)],
                         ids=["plain", "min_new_tokens", "ngram", "min_p"])
@pytest.mark.parametrize("rep", [1.0, 2.0])
@pytest.mark.parametrize("top_k,top_p", [(15, 0.85), (0, 1.0), (50, 0.7)])
def test_accept_sample_matches_oracle(top_k, top_p, rep, kw):
    from genvc_amd.engine import logits_processors, sample_params, spec_accept_sample
    c = accept_case(top_k, top_p, rep, kw)
    out, ref = c["out"], c["ref"]
    floor = min(out["margins"])
    print(f"seed {c['seed']}: {out['accepts']} accepts, {out['rejects']} rejections, smallest margin {floor:.3e}")
    assert floor > MARGIN, "no seed in the searched range clears the margins"
    # what the rows were planted for, on the oracle
    assert out["accepts"] > 0 and out["rejects"] > 0
    kk = [min(K_ACC, MAX_NEW - e - 1) for e in EMITTED]
    assert kk[5] == 2 and any(ref["accepted"][b] == kk[b] and ref["drafted"][b] == kk[b] and kk[b] > 0 for b in range(B_ACC))
    assert ref["accepted"][6] == K_ACC                                                           # p == q accepts every draft
    assert c["drafts"][STOP_ROW, STOP_AT] == EOS
    assert ref["rounds"][4] == 0 and ref["drop_target"][4] == K_ACC + 1 and ref["emitted"][4] == EMITTED[4]      # the finished row
    st = make_state(c["base"], K_ACC)
    params = sample_params(c["samp"], V, EOS, c["seed"])
    proc = logits_processors(c["kw"], N0, V, sampling=True)
    assert (proc is None) == (not c["kw"])
    p_rows = spec_accept_sample(st, K_ACC, K_ACC + 1, c["logits"].to(DEV), c["latents"].to(DEV), torch.from_numpy(c["drafts"]).to(DEV),
                                torch.from_numpy(c["q"]).to(DEV), params, proc=proc)
    compare_state(st, ref)
    # the warped rows the kernel drew from keep the oracle's entries (scores to fp32 rounding of the same operations)
    got, want = p_rows.cpu().numpy(), out["p"]
    used = ~np.isnan(want[:, :, 0])
    assert used.sum() >= B_ACC - 1
    assert np.array_equal(np.isfinite(got[used]), np.isfinite(want[used]))
    fin = np.isfinite(want[used])
    assert np.abs(got[used][fin] - want[used][fin]).max() < 1e-5


def test_accept_sample_opening_step():
    """k = 0: token 0 of every row is drawn from p_0 with u_res(0); nothing is appended and no round is counted"""
    from genvc_amd.engine import sample_params, spec_accept_sample
    B = 4
    samp = dict(repetition_penalty=2.0, temperature=0.85, top_k=15, top_p=0.85)
    logits = synth.uniform(61, "spec_open", (B, 1, V), 2.0).float()
    logits[2, 0, EOS] = 40.0
    latents = synth.uniform(62, "spec_open_lat", (B, 1, D_LAT), 1.0).float()
    base = dict(ids=np.ones((B, N0 + MAX_NEW + 16), dtype=np.int32), ids_len=np.full(B, N0, dtype=np.int32),
                finished=np.zeros(B, dtype=np.int32), emitted=np.zeros(B, dtype=np.int32), pending=np.full(B, -1, dtype=np.int32),
                toks=np.full((B, MAX_NEW), EOS, dtype=np.int32), lats=np.zeros((B, MAX_NEW, D_LAT), dtype=np.float32),
                drop_target=np.zeros(B, dtype=np.int32), drop_assistant=np.zeros(B, dtype=np.int32), rounds=np.zeros(B, dtype=np.int32),
                drafted=np.zeros(B, dtype=np.int32), accepted=np.zeros(B, dtype=np.int32), max_new=MAX_NEW)
    for seed in range(500, 600):
        ref = {n: (v.copy() if isinstance(v, np.ndarray) else v) for n, v in base.items()}
        out = SO.accept(ref, 0, 0, logits.numpy(), latents.numpy(), None, None, samp, seed, EOS, {}, N0)
        if min(out["margins"]) > MARGIN:
            break
    assert min(out["margins"]) > MARGIN
    st = make_state(base, 3)
    spec_accept_sample(st, 0, 0, logits.to(DEV), latents.to(DEV), None, None, sample_params(samp, V, EOS, seed))
    compare_state(st, ref)
    assert ref["emitted"].tolist() == [1] * B and ref["finished"].tolist() == [0, 0, 1, 0] and ref["toks"][2, 0] == EOS
    assert ref["rounds"].tolist() == [0] * B and ref["drop_target"].tolist() == [0] * B
    assert len(set(ref["toks"][:, 0].tolist())) > 1          # rows draw with their own uniforms


def test_accept_sample_refuses_bad_arguments_on_the_host():
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import sample_params, spec_accept_sample
    c = accept_case(15, 0.85, 1.0, ())
    st = make_state(c["base"], K_ACC)
    args = (st, K_ACC, K_ACC + 1, c["logits"].to(DEV), c["latents"].to(DEV), torch.from_numpy(c["drafts"]).to(DEV))
    q = torch.from_numpy(c["q"]).to(DEV)
    for samp in (dict(c["samp"], top_k=V + 1), dict(c["samp"], temperature=0.0)):
        with pytest.raises(GenvcHipError):
            spec_accept_sample(*args, q, sample_params(samp, V, EOS, 0))
    with pytest.raises(GenvcHipError, match="null workspace"):
        spec_accept_sample(*args, None, sample_params(c["samp"], V, EOS, 0))
    torch.cuda.synchronize()
    compare_state(st, c["base"])          # nothing was launched


# ---- 2. the distribution of a round's first token --------------------------------------------------------------------------------------
@pytest.mark.parametrize("disjoint", [False, True], ids=["overlapping", "disjoint-top-k"])
def test_first_token_distribution(disjoint):
    """64 calls of B = 64, k = 1 (128 rows): the histogram of the 4096 first tokens against p_0 stays under the chi-square 0.999
    quantile, and every draw whose margins pass equals the oracle's (the screen leaves out at most 3 %; measured 0.12 % / 0.27 %).
    disjoint: the draft's 15 best ids are the target's 15 worst, nothing is accepted and the residual is p_0 itself"""
    from genvc_amd.engine import sample_params, spec_accept_sample
    case = SO.dist_case(disjoint)
    Vd, Bd = SO.DIST_V, SO.DIST_B
    logits = case["logits"].view(1, 2, Vd).expand(Bd, 2, Vd).contiguous().to(DEV)
    latents = torch.zeros(Bd, 2, 4, device=DEV)
    from genvc_amd.engine import AssistedState
    toks, want, clear, accepted = [], [], [], 0
    for seed in SO.DIST_SEEDS:
        drafts, q, t, floor, acc, p = SO.dist_round(case, seed)
        st = AssistedState(torch.ones(Bd, SO.DIST_N0, dtype=torch.int32, device=DEV), 1, 4, SO.DIST_EOS, Vd, 4)
        st.ids[:, SO.DIST_N0] = 0          # the opening token of dist_round's row
        st.ids_len.fill_(SO.DIST_N0 + 1)
        st.emitted.fill_(1)
        spec_accept_sample(st, 1, 2, logits, latents, torch.from_numpy(drafts).to(DEV), torch.from_numpy(q).to(DEV),
                           sample_params(case["samp"], Vd, SO.DIST_EOS, seed))
        toks.append(st.toks[:, 1].cpu().numpy())
        accepted += int(st.accepted.sum())
        want.append(t)
        clear.append(floor > MARGIN)
    toks, want, clear = np.concatenate(toks), np.concatenate(want), np.concatenate(clear)
    c, dof, emin, outside = SO.chi2(toks, p)
    bound = SO.chi2_bound(dof)
    print(f"chi2 {c:.1f} on {dof} degrees of freedom (bound {bound:.1f}), smallest expected count {emin:.1f}, accepted {accepted}, "
          f"screened out {100.0 * (~clear).mean():.2f} %, differing from the oracle {int((toks != want).sum())}")
    assert len(toks) == 4096 and emin >= 10.0 and outside == 0
    assert c < bound
    assert (~clear).mean() <= 0.03
    assert np.array_equal(toks[clear], want[clear])
    assert accepted == 0 if disjoint else accepted > 0


# ---- 3. whole generations against the oracle chain --------------------------------------------------------------------------------------
SAMP = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0)


def weights(model_args, seed):
    return synth.make_weights(seed, synth.gpt_weight_spec(gcfg.gpt_dims(model_args)))


def make_gpt(model_args, seed, max_slots=8):
    from genvc_amd.layers.gpt import GPT
    a = model_args
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    g.load_state_dict(weights(a, seed), strict=False)
    g.to(DEV)
    g.init_gpt_for_inference(max_slots=max_slots)
    g.max_gen_mel_tokens = MAX_NEW
    return g


def inputs(dims, b):
    return (synth.uniform(IN_SEED, "cond_latents", (b, 32, dims["d_model"]), 1.0), synth.integers(IN_SEED, "content_codes", (b, TC), 256))


def close(*gs):
    for g in gs:
        g.engine.close()
    torch.cuda.empty_cache()


_chain = {}


def chain(targs, tseed, dargs, dseed, b, k, seed):
    """the oracle chain of one case at one RNG seed, computed once and shared (read-only)"""
    key = (id(targs), tseed, id(dargs), dseed, b, k, seed)
    if key not in _chain:
        cond, codes = inputs(gcfg.gpt_dims(targs), b)
        _chain[key] = SO.generate(weights(targs, tseed), gcfg.gpt_dims(targs), weights(dargs, dseed), gcfg.gpt_dims(dargs), cond, codes, k,
                                  SAMP, seed, MAX_NEW, logit_screen=LOGIT_SCREEN, logit_tol=TOL)
    return _chain[key]


# (target, its model seed, draft, its model seed, streams, k, the call's RNG seed).  The RNG seeds are the first from 0 that pass the screen
# of SO.generate, found on the CPU with need=MARGIN and asserted below: every decision keeps a margin above MARGIN when the logits of
# both models move by up to LOGIT_SCREEN (draws from a warped row, accept tests) or by up to TOL, the tolerance the device's logits
# are held to against the oracle's (residual draws, TopK's last gap, TopP's cut).  The 2e-3 screen cannot cover the second group: a
# worst-case 2e-3 move of every logit shifts a residual CDF by several percent and closes TopK's last gap in about one row in eight,
# and of 100 seeds none passed either check over a generation's ~40 warped rows (draws and accept tests alone: 39 passed; with TOL
# for the rest: 20 of 100 per row).  Unrelated drafts are never accepted at top_k = 15 (the two models' kept sets hardly meet); the
# self-draft case is where the chain accepts
GEN_CASES = [("tiny-unrelated", TINY, 0, TINY, 5, 1, 3, 12), ("tiny-unrelated", TINY, 0, TINY, 5, 2, 3, 215),
             ("tiny4-shallow", TINY4, 1, TINY, 6, 1, 3, 22), ("tiny4-shallow", TINY4, 1, TINY, 6, 2, 3, 440),
             ("tiny-self", TINY, 0, TINY, 0, 2, 3, 8), ("full2-rows-step", FULL2, 0, FULL2, 5, 2, 7, 254)]


@pytest.mark.parametrize("name,targs,tseed,dargs,dseed,b,k,seed", GEN_CASES, ids=[f"{c[0]}-B{c[5]}" for c in GEN_CASES])
def test_generation_matches_oracle_chain(name, targs, tseed, dargs, dseed, b, k, seed):
    r = chain(targs, tseed, dargs, dseed, b, k, seed)
    print(f"oracle: ids {r['ids'].tolist()} rounds {r['rounds'].tolist()} drafted {r['drafted'].tolist()} accepted "
          f"{r['accepted'].tolist()}, smallest margin less the logit allowance {r['floor']:.3e}")
    assert r["floor"] > MARGIN, "the case is not margin-screened"
    g, asst = make_gpt(targs, tseed), make_gpt(dargs, dseed)
    cond, codes = inputs(gcfg.gpt_dims(targs), b)
    ids = g.generate(cond.to(DEV), codes.to(DEV), assistant_model=asst, speculative_sampling=True, num_assistant_tokens=k, seed=seed,
                     **SAMP).cpu().numpy()
    stats = {n: t.cpu().numpy() for n, t in g.last_assist_stats.items()}
    print(f"device: ids {ids.tolist()} stats {({n: v.tolist() for n, v in stats.items()})}")
    if name.startswith("full2"):
        assert g.engine.decode_variant() == 5
    assert np.array_equal(ids, r["ids"])
    for n in ("rounds", "drafted", "accepted"):
        assert np.array_equal(stats[n], r[n]), n
    if name == "tiny-self":
        assert np.array_equal(r["accepted"], r["drafted"]) and r["accepted"].sum() > 0          # the chain that accepts
    lens = [int(np.nonzero(row == EOS)[0][0]) + 1 if (row == EOS).any() else len(row) for row in ids]
    lat = g.last_latents.cpu()
    err = max(float((lat[i, :n] - r["latents"][i, :n]).abs().max()) for i, n in enumerate(lens))
    print(f"latent err {err:.3e}")
    assert err < TOL
    lp, ln = g.sequence_logprobs(torch.from_numpy(ids).to(DEV), g.last_latents)          # keeps working on the returned tokens and latents
    assert ln.tolist() == lens and bool(torch.isfinite(lp).all())
    close(g, asst)


# ---- 4. self-draft, split rounds, isolation, refusal --------------------------------------------------------------------------------------
def test_self_draft_accepts_everything():
    """an assistant with the target's own weights: p / q differs from 1 only through the two paths' logits (1e-4 apart at most, which
    the repetition penalty and the temperature stretch to 2 * 2.0 * 1e-4 / 0.85 < 1e-3 on a probability ratio), so a rejection needs
    u_acc within 1e-3 of 1: the RNG seed is the first whose accept uniforms all stay below 1 - 1e-3"""
    b, k = 2, 3
    seed = next(s for s in range(100) if all(SO.u_acc(s, t, r) < 1.0 - 1e-3 for t in range(MAX_NEW) for r in range(b)))
    assert all(SO.u_acc(seed, t, r) < 1.0 - 1e-3 for t in range(MAX_NEW) for r in range(b))
    g, asst = make_gpt(TINY, 0), make_gpt(TINY, 0)
    cond, codes = inputs(gcfg.gpt_dims(TINY), b)
    ids = g.generate(cond.to(DEV), codes.to(DEV), assistant_model=asst, speculative_sampling=True, num_assistant_tokens=k, seed=seed, **SAMP)
    s = {n: t.cpu().numpy() for n, t in g.last_assist_stats.items()}
    print(f"seed {seed}: ids {ids.tolist()} stats {({n: v.tolist() for n, v in s.items()})}")
    assert ids.shape[1] == MAX_NEW or bool((ids == EOS).any(1).all())
    assert np.array_equal(s["accepted"], s["drafted"]) and s["drafted"].sum() > 0
    close(g, asst)


def test_split_rounds_and_isolation():
    """position-keyed uniforms: one round per host check gives the tokens of sixteen; and a plain sampled call, a greedy assisted call
    and a plain call again around the sampled assisted call return what they return alone"""
    g, asst = make_gpt(TINY, 0), make_gpt(TINY, 5)
    cond, codes = inputs(gcfg.gpt_dims(TINY), 2)
    cond, codes = cond.to(DEV), codes.to(DEV)
    plain = g.generate(cond, codes, seed=4, **SAMP)
    greedy = g.generate(cond, codes, do_sample=False, repetition_penalty=2.0, assistant_model=asst, num_assistant_tokens=3)
    kw = dict(assistant_model=asst, speculative_sampling=True, num_assistant_tokens=3, seed=4, **SAMP)
    one = g.generate(cond, codes, group=16, **kw)
    s1 = {n: t.clone() for n, t in g.last_assist_stats.items()}
    assert torch.equal(plain, g.generate(cond, codes, seed=4, **SAMP))
    many = g.generate(cond, codes, group=1, **kw)
    assert torch.equal(one, many) and all(torch.equal(s1[n], g.last_assist_stats[n]) for n in s1)
    assert torch.equal(greedy, g.generate(cond, codes, do_sample=False, repetition_penalty=2.0, assistant_model=asst, num_assistant_tokens=3))
    assert torch.equal(greedy, g.generate(cond, codes, do_sample=False, repetition_penalty=2.0))          # (assisted greedy = plain greedy)
    assert torch.equal(plain, g.generate(cond, codes, seed=4, **SAMP))
    assert torch.equal(one, g.generate(cond, codes, group=16, **kw))
    # the draft context serves its own plain calls as before
    a1 = asst.generate(cond, codes, seed=4, **SAMP)
    g.generate(cond, codes, **kw)
    assert torch.equal(a1, asst.generate(cond, codes, seed=4, **SAMP))
    close(g, asst)


def test_a_call_without_the_kwarg_is_refused_and_leaves_the_slots_usable():
    g, asst = make_gpt(TINY, 0), make_gpt(TINY, 5)
    cond, codes = inputs(gcfg.gpt_dims(TINY), 2)
    cond, codes = cond.to(DEV), codes.to(DEV)
    before = g.generate(cond, codes, seed=4, **SAMP)
    with pytest.raises(NotImplementedError, match="speculative_sampling=True"):
        g.generate(cond, codes, assistant_model=asst, seed=4, **SAMP)
    assert torch.equal(before, g.generate(cond, codes, seed=4, **SAMP))
    out = g.generate(cond, codes, assistant_model=asst, speculative_sampling=True, seed=4, **SAMP)
    assert out.shape[0] == 2 and 1 <= out.shape[1] <= MAX_NEW
    g.engine.health()
    asst.engine.health()
    close(g, asst)
