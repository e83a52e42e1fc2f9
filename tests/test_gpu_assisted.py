"""GPU: assisted (speculative) greedy decoding (GPT.generate(assistant_model=...); include/genvc_hip.h: gvc_gpt_verify,
gvc_gpt_truncate, gvc_spec_accept, gvc_gpt_generate_assisted).
1. the multi-row verification pass against the same tokens fed one gvc_gpt_decode_step at a time to copies of the slots, and the
   rollback;  2. the accept kernel against its numpy restatement (tests/assist_oracle.py), every output exactly;  3. assisted greedy
   ids bit for bit against the CPU oracle's plain greedy ids and against the same GPT's call without the assistant, on margin-screened
   cases (the project's 2e-3 logit screen times the repetition penalty, asserted on the oracle's own margins first)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assist_oracle as AO                    # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026
MAX_NEW = 12
IN_SEED = 13         # input seed of every case; the model seeds below pass the screen with it (checked on the CPU)
TC = 6
TINY = gcfg.TINY_MODEL_ARGS
TINY4 = dict(gcfg.TINY_MODEL_ARGS, gpt_layers=4)         # a target one layer pair deeper than a TINY assistant
FULL2 = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2)      # the default widths with two layers: the oracle stays quick
TOL = 1e-4           # the project's logit and latent tolerance


def weights(model_args, seed, stop_bias=None):
    w = synth.make_weights(seed, synth.gpt_weight_spec(gcfg.gpt_dims(model_args)))
    if stop_bias is not None:
        w["mel_head.bias"][EOS] = float(stop_bias)
    return w


def make_gpt(model_args, seed, stop_bias=None, max_slots=8):
    from genvc_amd.layers.gpt import GPT
    a = model_args
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    g.load_state_dict(weights(a, seed, stop_bias), strict=False)
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


# ---- 1. the verification pass against sequential decode steps, and the rollback -------------------------------------------------
@pytest.mark.parametrize("T", [1, 4, 7, 9])
@pytest.mark.parametrize("model", ["tiny", "full2"])
def test_verify_matches_sequential_decode_steps(model, T):
    """B = 2 slots at different cached lengths (slot 0 has decoded one token more than its prefill).  Slots 2, 3 are copies that are
    fed the same tokens one decode step at a time; slot 4 is a copy of slot 0 as its prefill left it, fed what slot 0 keeps after the
    rollback.  At FULL2 2 x 7 = 14 rows run on the one-launch rows step and 2 x 9 = 18 on the skinny path; TINY takes the skinny path.
    The lengths are not readable from outside: a slot that stood anywhere but at base + T (or base + T - drop) would attend to other
    keys at another position in the step that follows, which is compared too."""
    args = TINY if model == "tiny" else FULL2
    dims = gcfg.gpt_dims(args)
    g = make_gpt(args, 0)
    eng = g.engine
    cond, codes = inputs(dims, 2)
    g.compute_embeddings(cond.to(DEV), codes.to(DEV))

    def sl(*i):
        return torch.tensor(i, device=DEV, dtype=torch.int32)
    gen = torch.Generator().manual_seed(100 + T)
    toks = torch.randint(0, 1024, (2, T), generator=gen).to(torch.int32).to(DEV)
    extra = torch.tensor([7], dtype=torch.int32, device=DEV)
    nxt = torch.tensor([11, 12], dtype=torch.int32, device=DEV)
    eng.prefill(sl(0, 1), g._prefix)
    eng.kv_fanout(sl(0), sl(4))
    eng.decode_step(sl(0), extra)
    eng.kv_fanout(sl(0, 1), sl(2, 3))
    vl, vz = eng.verify(sl(0, 1), toks)
    variant = eng.decode_variant()
    seq = [eng.decode_step(sl(2, 3), toks[:, t].contiguous()) for t in range(T)]
    sl_, sz = torch.stack([a for a, _ in seq], 1), torch.stack([b for _, b in seq], 1)
    e_l, e_z = float((vl - sl_).abs().max()), float((vz - sz).abs().max())
    print(f"{model} T {T}: variant {variant}, logits err {e_l:.3e}, latent err {e_z:.3e} (tolerance {TOL:.0e})")
    assert variant == (5 if model == "full2" and 2 * T <= 16 else 4)
    assert e_l < TOL and e_z < TOL
    # rollback by [2, 0]: slot 0 keeps T - 1 of the T + 1 tokens behind its prefill; slot 4 is fed exactly those
    eng.truncate(sl(0, 1), torch.tensor([2, 0], dtype=torch.int32, device=DEV))
    kept = torch.cat([extra, toks[0]])[:T - 1]
    for t in kept:
        eng.decode_step(sl(4), t.view(1).contiguous())
    al, az = eng.decode_step(sl(0, 1), nxt)
    bl, bz = eng.decode_step(sl(4, 3), nxt)
    e_l, e_z = float((al - bl).abs().max()), float((az - bz).abs().max())
    print(f"  after truncate [2, 0]: logits err {e_l:.3e}, latent err {e_z:.3e}")
    assert e_l < TOL and e_z < TOL
    eng.health()
    close(g)


def test_verify_refuses_more_than_128_rows():
    from genvc_amd._lib import GenvcHipError
    g = make_gpt(TINY, 0, max_slots=16)
    slots = torch.arange(9, device=DEV, dtype=torch.int32)
    with pytest.raises(GenvcHipError, match="128 rows"):
        g.engine.verify(slots, torch.zeros(9, 15, dtype=torch.int32, device=DEV))
    close(g)


# ---- 2. the accept kernel against its numpy restatement ---------------------------------------------------------------------------
K_ACC, N0 = 4, 9
# (emitted so far, drafts that agree, stop token planted at this position or None, already finished)
ACC_ROWS = [(3, 0, None, 0), (1, 2, None, 0), (5, K_ACC, None, 0), (2, K_ACC, 1, 0), (4, 1, None, 1), (MAX_NEW - 2, K_ACC, None, 0),
            (MAX_NEW - 1, 2, None, 0)]


def accept_case(rep, kw):
    """random logits with planted drafts: row b's first `agree` drafts are the chain's own tokens, the next one is not"""
    from genvc_amd.engine import AssistedState
    B, k = len(ACC_ROWS), K_ACC
    gen = torch.Generator().manual_seed(5)
    logits = (torch.rand(B, k + 1, V, generator=gen) * 8 - 4).float()
    latents = torch.rand(B, k + 1, 8, generator=gen).float()
    if kw.get("suppress_tokens"):
        logits[:, :, 3] = 30.0          # the suppressed id would win every position
    if kw.get("min_new_tokens"):
        logits[1, 0, EOS] = 50.0        # row 1 has emitted one token: its stop token is still banned
    st = AssistedState(torch.ones(B, N0, dtype=torch.int32, device=DEV), k, MAX_NEW, EOS, V, 8)
    ids = st.ids.cpu().numpy()
    drafts = np.zeros((B, k), dtype=np.int32)
    for b, (em, agree, stop_at, fin) in enumerate(ACC_ROWS):
        ids[b, N0:N0 + em] = torch.randint(0, 1024, (em,), generator=gen).numpy()
        if stop_at is not None:
            logits[b, stop_at, EOS] = 50.0
        row = [int(x) for x in ids[b, :N0 + em]]
        for i in range(k):
            tok, _ = AO.chain_token(logits[b, i], row, N0, kw, rep, EOS)
            drafts[b, i] = tok if i < agree else (tok + 1) % 1024
            row.append(int(drafts[b, i]))
    em = np.array([r[0] for r in ACC_ROWS], dtype=np.int32)
    ref = dict(ids=ids.copy(), ids_len=N0 + em, finished=np.array([r[3] for r in ACC_ROWS], dtype=np.int32), emitted=em.copy(),
               pending=np.full(B, -1, dtype=np.int32), toks=np.full((B, MAX_NEW), EOS, dtype=np.int32),
               lats=np.zeros((B, MAX_NEW, 8), dtype=np.float32), drop_target=np.zeros(B, dtype=np.int32),
               drop_assistant=np.zeros(B, dtype=np.int32), rounds=np.zeros(B, dtype=np.int32), drafted=np.zeros(B, dtype=np.int32),
               accepted=np.zeros(B, dtype=np.int32), max_new=MAX_NEW)
    st.ids.copy_(torch.from_numpy(ids))
    st.ids_len.copy_(torch.from_numpy(ref["ids_len"]))
    st.finished.copy_(torch.from_numpy(ref["finished"]))
    st.emitted.copy_(torch.from_numpy(ref["emitted"]))
    return st, ref, logits, latents, drafts


def compare_state(st, ref):
    for name in ("ids", "ids_len", "finished", "emitted", "pending", "toks", "lats", "drop_target", "drop_assistant", "rounds", "drafted",
                 "accepted"):
        got = getattr(st, name).cpu().numpy()
        assert np.array_equal(got, ref[name]), (name, got, ref[name])


@pytest.mark.parametrize("kw", [{}, {"min_new_tokens": 3}, {"suppress_tokens": [3, 500, 1000]}, {"no_repeat_ngram_size": 2}],
                         ids=["plain", "min_new_tokens", "suppress_tokens", "ngram"])
@pytest.mark.parametrize("rep", [1.0, 2.0])
def test_accept_matches_numpy(rep, kw):
    from genvc_amd.engine import logits_processors, sample_params, spec_accept
    st, ref, logits, latents, drafts = accept_case(rep, kw)
    params = sample_params(dict(repetition_penalty=rep, temperature=1.0, top_p=1.0, top_k=1), V, EOS)
    proc = logits_processors(kw, N0, V, sampling=False)
    assert (proc is None) == (not kw)
    spec_accept(st, K_ACC, K_ACC + 1, logits.to(DEV), latents.to(DEV), torch.from_numpy(drafts).to(DEV), params, proc=proc)
    AO.accept(ref, K_ACC, K_ACC + 1, logits.numpy(), latents.numpy(), drafts, rep, EOS, kw, N0)
    compare_state(st, ref)
    # what the rows were planted for
    assert list(ref["accepted"][:3]) == [0, 2, K_ACC] and list(ref["drafted"][:3]) == [K_ACC] * 3
    assert ref["toks"][3, 2 + 1] == EOS and ref["finished"][3] == 1 and ref["emitted"][3] == 2 + 2          # the planted stop token
    assert ref["emitted"][4] == 4 and ref["drop_target"][4] == K_ACC + 1 and ref["rounds"][4] == 0           # the finished row
    assert ref["emitted"][5] == MAX_NEW and ref["finished"][5] == 1 and ref["drafted"][5] == 1               # the budget ends mid-round
    assert ref["emitted"][6] == MAX_NEW and ref["drafted"][6] == 0 and ref["drop_target"][6] == K_ACC        # one token to go
    if kw.get("suppress_tokens"):
        assert not (ref["toks"] == 3).any()
    if kw.get("min_new_tokens"):
        assert ref["toks"][1, 1] != EOS


def test_accept_opening_step():
    """k = 0: one target token per row from one logits row, nothing appended, no round counted"""
    from genvc_amd.engine import AssistedState, sample_params, spec_accept
    B = 3
    gen = torch.Generator().manual_seed(6)
    logits = (torch.rand(B, 1, V, generator=gen) * 8 - 4).float()
    logits[2, 0, EOS] = 50.0
    latents = torch.rand(B, 1, 8, generator=gen).float()
    st = AssistedState(torch.ones(B, N0, dtype=torch.int32, device=DEV), 3, MAX_NEW, EOS, V, 8)
    params = sample_params(dict(repetition_penalty=2.0, temperature=1.0, top_p=1.0, top_k=1), V, EOS)
    spec_accept(st, 0, 0, logits.to(DEV), latents.to(DEV), None, params)
    want = [AO.chain_token(logits[b, 0], [1] * N0, N0, {}, 2.0, EOS)[0] for b in range(B)]
    assert st.toks[:, 0].tolist() == want and st.pending.tolist() == want and want[2] == EOS
    assert st.emitted.tolist() == [1] * B and st.ids_len.tolist() == [N0 + 1] * B and st.finished.tolist() == [0, 0, 1]
    assert st.drop_target.tolist() == [0] * B and st.rounds.tolist() == [0] * B and st.drafted.tolist() == [0] * B
    assert torch.equal(st.lats[:, 0].cpu(), latents[:, 0])


# ---- 3. assisted greedy equals plain greedy ----------------------------------------------------------------------------------------
_oracle = {}


def oracle(model_args, seed, b, rep=1.0, kw=None, stop_bias=None):
    """the CPU oracle's plain greedy decoding of one case, computed once per session and shared (read-only)"""
    key = (id(model_args), seed, b, rep, repr(sorted((kw or {}).items())), stop_bias)
    if key not in _oracle:
        dims = gcfg.gpt_dims(model_args)
        ora = AO.BO.OracleGpt(weights(model_args, seed, stop_bias), dims)
        cond, codes = inputs(dims, b)
        _oracle[key] = AO.greedy(ora, cond, codes, kw, rep, MAX_NEW)
    return _oracle[key]


def screen(r, rep):
    m = r["margins"]
    floor = float(m[np.isfinite(m)].min())
    need = rep * 2e-3
    print(f"oracle margin {floor:.3e} (screen {need:.1e})")
    assert floor >= need, f"case is not margin-screened: {floor:.3e} < {need:.1e}"


def row_lengths(ids):
    """tokens each row emitted: up to and including its first stop token"""
    return [int(np.nonzero(row == EOS)[0][0]) + 1 if (row == EOS).any() else len(row) for row in ids]


def check_assisted(g, asst, r, b, k, rep=1.0, kw=None, plain=None, own=False, rows_step=False):
    cond, codes = inputs(g.engine.dims, b)
    more = dict(kw or {})
    ids = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False, repetition_penalty=rep, assistant_model=asst,
                     num_assistant_tokens=k, **more).cpu().numpy()
    stats = {n: t.cpu().numpy() for n, t in g.last_assist_stats.items()}
    print(f"B {b} k {k}: rounds {stats['rounds'].tolist()} drafted {stats['drafted'].tolist()} accepted {stats['accepted'].tolist()}")
    if rows_step:
        assert g.engine.decode_variant() == 5
    assert np.array_equal(ids, r["ids"])
    if plain is not None:
        assert np.array_equal(ids, plain)
    lens = row_lengths(ids)
    lat = g.last_latents.cpu()
    assert lat.shape[:2] == ids.shape
    err = max(float((lat[i, :n] - r["latents"][i, :n]).abs().max()) for i, n in enumerate(lens))
    print(f"  latent err {err:.3e}")
    assert err < TOL
    assert all(t.dtype == torch.int64 and tuple(t.shape) == (b,) for t in g.last_assist_stats.values())
    assert (stats["accepted"] <= stats["drafted"]).all() and (stats["drafted"] <= k * stats["rounds"]).all()
    if own:
        # the target's own weights: every compared draft is accepted, and a row of n tokens (token 0 comes from the opening step,
        # which counts no round) ran ceil((n - 1) / (k + 1)) rounds
        assert np.array_equal(stats["accepted"], stats["drafted"])
        assert stats["rounds"].tolist() == [math.ceil((n - 1) / (k + 1)) for n in lens]
    return stats


GEN_CASES = [("tiny", TINY, 0, "own"), ("tiny", TINY, 0, "seed"), ("tiny4", TINY4, 1, "shallow"), ("full2", FULL2, 0, "own"),
             ("full2", FULL2, 0, "seed")]


@pytest.mark.parametrize("b", [1, 2])
@pytest.mark.parametrize("name,args,seed,kind", GEN_CASES, ids=[f"{c[0]}-{c[3]}" for c in GEN_CASES])
def test_assisted_greedy_equals_plain_greedy(name, args, seed, kind, b):
    """assistants: the target's own weights (everything accepted), another model seed (most drafts rejected), and a model one layer
    pair shallower (a 2-layer TINY drafting for a 4-layer target).  k = 1, 3, 7 on one pair of contexts"""
    r = oracle(args, seed, b)
    screen(r, 1.0)
    g = make_gpt(args, seed)
    asst = make_gpt(args, seed) if kind == "own" else make_gpt(TINY if kind == "shallow" else args, seed + 5)
    cond, codes = inputs(gcfg.gpt_dims(args), b)
    plain = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False).cpu().numpy()
    assert not hasattr(g, "last_assist_stats")
    rates = []
    for k in (1, 3, 7):
        s = check_assisted(g, asst, r, b, k, plain=plain, own=kind == "own", rows_step=name == "full2")
        rates.append(s["accepted"].sum() / max(1, s["drafted"].sum()))
    if kind == "seed":
        assert max(rates) < 0.5          # an unrelated model: most drafts are rejected
    again = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False).cpu().numpy()
    assert np.array_equal(again, plain)
    close(g, asst)


def test_a_row_ends_inside_a_round_while_the_other_goes_on():
    """stop bias 2.46 on model seed 3: the oracle's row 0 stops at its second token, row 1 at its eleventh"""
    seed, sb = 3, 2.46
    r = oracle(TINY, seed, 2, stop_bias=sb)
    screen(r, 1.0)
    assert row_lengths(r["ids"]) == [2, 11]
    g, asst = make_gpt(TINY, seed, stop_bias=sb), make_gpt(TINY, seed, stop_bias=sb)
    cond, codes = inputs(gcfg.gpt_dims(TINY), 2)
    plain = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False).cpu().numpy()
    for k in (3, 7):
        s = check_assisted(g, asst, r, 2, k, plain=plain)
        assert s["rounds"][0] == 1 and s["rounds"][1] == math.ceil(10 / (k + 1))
    close(g, asst)


def test_repetition_penalty_and_ngram_processor():
    seed, rep, kw = 2, 2.0, dict(no_repeat_ngram_size=2)
    r = oracle(TINY, seed, 2, rep=rep, kw=kw)
    screen(r, rep)
    bare = oracle(TINY, seed, 2)
    assert not np.array_equal(r["ids"], bare["ids"])          # the settings change the tokens
    g, own, other = make_gpt(TINY, seed), make_gpt(TINY, seed), make_gpt(TINY, seed + 5)
    cond, codes = inputs(gcfg.gpt_dims(TINY), 2)
    plain = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False, repetition_penalty=rep, **kw).cpu().numpy()
    check_assisted(g, own, r, 2, 3, rep=rep, kw=kw, plain=plain, own=True)
    check_assisted(g, other, r, 2, 3, rep=rep, kw=kw, plain=plain)
    close(g, own, other)


def test_plain_one_stream_calls_around_an_assisted_call():
    """a plain one-stream generate leaves a deferred token in its slot; the assisted call on the same contexts settles it, and the
    plain call afterwards returns what it returned before (on the target and on the context that drafted)"""
    r = oracle(TINY, 0, 1)
    screen(r, 1.0)
    g, asst = make_gpt(TINY, 0), make_gpt(TINY, 5)
    cond, codes = inputs(gcfg.gpt_dims(TINY), 1)
    first = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False)
    assert g.engine.decode_variant() == 3                       # the one-stream step: the call deferred its last decode
    lat1 = g.last_latents.clone()
    afirst = asst.generate(cond.to(DEV), codes.to(DEV), do_sample=False)
    check_assisted(g, asst, r, 1, 3, plain=first.cpu().numpy())
    again = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False)
    assert torch.equal(first, again) and torch.equal(lat1, g.last_latents)
    assert torch.equal(afirst, asst.generate(cond.to(DEV), codes.to(DEV), do_sample=False))
    close(g, asst)


def test_split_rounds_continue_exactly():
    """the host looks at the finished flags once per group // (k + 1) rounds: one round per call gives the same tokens"""
    r = oracle(TINY, 0, 2)
    g, asst = make_gpt(TINY, 0), make_gpt(TINY, 5)
    cond, codes = inputs(gcfg.gpt_dims(TINY), 2)
    kw = dict(do_sample=False, assistant_model=asst, num_assistant_tokens=3)
    one = g.generate(cond.to(DEV), codes.to(DEV), group=64, **kw)
    s1 = {n: t.clone() for n, t in g.last_assist_stats.items()}
    many = g.generate(cond.to(DEV), codes.to(DEV), group=1, **kw)
    assert torch.equal(one, many) and np.array_equal(one.cpu().numpy(), r["ids"])
    assert all(torch.equal(s1[n], g.last_assist_stats[n]) for n in s1)
    close(g, asst)
