"""GPU: classifier-free guidance (GPT.generate(guidance_scale=s, negative_cond_latents=...); include/genvc_hip.h: gvc_cfg_guide,
gvc_gpt_generate_cfg) against tests/cfg_oracle.py -- the oracle's two GPT forwards combined by the installed transformers' own
UnbatchedClassifierFreeGuidanceLogitsProcessor, executed, followed by HF's own processor objects.  Greedy ids are compared bit for bit on
margin-screened cases: the screen is the project's 2e-3 logit screen times the error amplification of the chain, rep * (2s - 1)
(|s| + |s - 1| = 2s - 1 for the combine at s > 1, times the repetition penalty's factor), and every test asserts it on the oracle's own
margins before it compares."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_oracle as CF                       # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026
MAX_NEW = 12
IN_SEED = 13         # input seed of every case: screened on the CPU so that model seeds 0, 2 (s = 1.5) and 0, 6 (s = 3, rep 2) pass
B, TC, TC_NEG = 2, 6, 9


def make_gpt(model_args, seed, stop_bias=None, max_slots=8):
    from genvc_amd.layers.gpt import GPT
    a = model_args
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    dims = gcfg.gpt_dims(a)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][EOS] = float(stop_bias)
    g.load_state_dict(w, strict=False)
    g.to(DEV)
    g.init_gpt_for_inference(max_slots=max_slots)
    g.max_gen_mel_tokens = MAX_NEW
    return g


def inputs(dims, in_seed=None, b=B, tc=TC, tc_neg=TC_NEG):
    """(cond, codes, negative cond, negative codes) on the CPU: the negatives come from input seed + 100 and have their own code length"""
    s = IN_SEED if in_seed is None else in_seed
    d = dims["d_model"]
    return (synth.uniform(s, "cond_latents", (b, 32, d), 1.0), synth.integers(s, "content_codes", (b, tc), 256),
            synth.uniform(s + 100, "cond_latents", (b, 32, d), 1.0), synth.integers(s + 100, "content_codes", (b, tc_neg), 256))


_oracle = {}


def oracle(model_args, seed, scale, rep, kw=None, stop_bias=None, b=B, in_seed=None):
    """the CPU restatement of one greedy case, computed once per session and shared (read-only) by the tests that need it"""
    key = (id(model_args), seed, scale, rep, repr(sorted((kw or {}).items())), stop_bias, b, in_seed)
    if key not in _oracle:
        dims = gcfg.gpt_dims(model_args)
        w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
        if stop_bias is not None:
            w["mel_head.bias"][EOS] = float(stop_bias)
        ora = CF.BO.OracleGpt(w, dims)
        cond, codes, ncond, ncodes = inputs(dims, in_seed, b)
        r = CF.guided(ora, cond, codes, ncond, ncodes, scale, rep=rep, kw=kw, max_new=MAX_NEW)
        r["unguided"] = CF.unguided(ora, cond, codes, rep=rep, max_new=MAX_NEW)
        r["ora"] = ora
        _oracle[key] = r
    return _oracle[key]


def screen(r, scale, rep):
    """the oracle's smallest top-1 / top-2 margin of the final scores against the screen: 2e-3 times the chain's amplification"""
    m = r["margins"]
    floor = float(m[np.isfinite(m)].min())
    need = rep * (2 * scale - 1) * 2e-3
    print(f"oracle margin {floor:.3e} (screen {need:.1e})")
    assert floor >= need, f"case is not margin-screened: {floor:.3e} < {need:.1e}"


def greedy_kw(scale, rep, ncond, ncodes, **more):
    return dict(do_sample=False, repetition_penalty=rep, guidance_scale=scale, negative_cond_latents=ncond.to(DEV),
                negative_text_inputs=ncodes.to(DEV), **more)


def close(g):
    g.engine.close()
    del g
    torch.cuda.empty_cache()


# ---- 1. the combine kernel against torch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("scale", [0.5, 1.5, 3.0])
@pytest.mark.parametrize("mag", [10.0, 300.0])
def test_cfg_guide_matches_torch(rows, scale, mag):
    from genvc_amd.engine import GptEngine
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=2)
    gen = torch.Generator().manual_seed(17)
    cond = (torch.rand(rows, V, generator=gen) * 2 - 1) * mag          # uniform in +-10, and the same scaled x30
    uncond = (torch.rand(rows, V, generator=gen) * 2 - 1) * mag
    tol = 1e-4 * (abs(scale) + abs(scale - 1))          # the project's logit tolerance times the combine's error amplification
    got = eng.cfg_guide(cond.to(DEV), uncond.to(DEV), scale).cpu()
    want = CF.closed_form(cond, uncond, scale)
    err = float((got - want).abs().max())
    print(f"rows {rows} scale {scale} mag {mag}: max abs err {err:.3e} (tolerance {tol:.1e})")
    assert torch.isfinite(got).all()
    assert err <= tol
    # cond == uncond: log_softmax(cond), whatever the scale
    same = eng.cfg_guide(cond.to(DEV), cond.to(DEV), scale).cpu()
    err = float((same - torch.log_softmax(cond, -1)).abs().max())
    print(f"  cond == uncond: max abs err {err:.3e}")
    assert torch.isfinite(same).all() and err <= tol
    eng.close()


# ---- 2. greedy guided ids bit-exact against the oracle, on both decode classes ----------------------------------------------------
GREEDY_CASES = [(1.5, 1.0, 0), (1.5, 1.0, 2), (3.0, 2.0, 0), (3.0, 2.0, 6)]


@pytest.mark.parametrize("one_launch", ["1", "0"], ids=["one_launch_steps", "launch_per_phase"])
@pytest.mark.parametrize("scale,rep,seed", GREEDY_CASES)
def test_guided_greedy_matches_oracle(scale, rep, seed, one_launch, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST_ROWS", one_launch)
    r = oracle(gcfg.TINY_MODEL_ARGS, seed, scale, rep)
    screen(r, scale, rep)
    g = make_gpt(gcfg.TINY_MODEL_ARGS, seed)
    cond, codes, ncond, ncodes = inputs(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS))
    ids = g.generate(cond.to(DEV), codes.to(DEV), **greedy_kw(scale, rep, ncond, ncodes)).cpu().numpy()
    assert np.array_equal(ids, r["ids"])
    err = float((g.last_latents.cpu() - r["latents"]).abs().max())
    print(f"latent err {err:.3e}")
    assert err < 1e-4
    # guidance changes the tokens: the same model without it decodes something else
    plain = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False, repetition_penalty=rep).cpu().numpy()
    assert plain.shape != ids.shape or not np.array_equal(plain, ids)
    close(g)


def test_guided_full_size_runs_on_the_rows_step():
    """the default widths (d_model 1024, 4 heads of 256; two layers, as smoke() runs them, so that the oracle stays quick): the 2B = 4
    rows of a guided call decode on the one-launch rows step (variant 5).  Model seed 1: seed 0 misses the screen at these widths
    (margin 1.4e-3 against 4e-3), seed 1 has 4.1e-2."""
    scale, rep, seed = 1.5, 1.0, 1
    r = oracle(FULL2, seed, scale, rep)
    screen(r, scale, rep)
    g = make_gpt(FULL2, seed)
    cond, codes, ncond, ncodes = inputs(gcfg.gpt_dims(FULL2))
    ids = g.generate(cond.to(DEV), codes.to(DEV), **greedy_kw(scale, rep, ncond, ncodes)).cpu().numpy()
    assert g.engine.decode_variant() == 5
    assert np.array_equal(ids, r["ids"])
    assert float((g.last_latents.cpu() - r["latents"]).abs().max()) < 1e-4
    close(g)


FULL2 = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2)      # the default widths with two layers: the oracle stays quick


# ---- 3. one item after a deferring call --------------------------------------------------------------------------------------------
def test_one_item_after_a_deferring_call():
    """an unguided one-stream generate leaves a pending token in its slot; the guided call that follows on the same context settles
    its slots first and equals the oracle, and the unguided call afterwards returns what it returned before"""
    scale, rep, seed = 1.5, 1.0, 0
    r = oracle(gcfg.TINY_MODEL_ARGS, seed, scale, rep, b=1)
    screen(r, scale, rep)
    g = make_gpt(gcfg.TINY_MODEL_ARGS, seed)
    cond, codes, ncond, ncodes = inputs(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), b=1)
    first = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False, repetition_penalty=rep)
    assert g.engine.decode_variant() == 3                       # the one-stream step: the call deferred its last decode
    lat1 = g.last_latents.clone()
    ids = g.generate(cond.to(DEV), codes.to(DEV), **greedy_kw(scale, rep, ncond, ncodes)).cpu().numpy()
    assert g.engine.decode_variant() != 3
    assert np.array_equal(ids, r["ids"])
    assert float((g.last_latents.cpu() - r["latents"]).abs().max()) < 1e-4
    again = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False, repetition_penalty=rep)
    assert torch.equal(first, again) and torch.equal(lat1, g.last_latents)
    close(g)


# ---- 4. a generation split into calls continues exactly --------------------------------------------------------------------------
def test_split_calls_continue_exactly():
    scale, rep, seed = 3.0, 2.0, 0
    g = make_gpt(gcfg.TINY_MODEL_ARGS, seed)
    cond, codes, ncond, ncodes = inputs(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS))
    one = g.generate(cond.to(DEV), codes.to(DEV), group=16, **greedy_kw(scale, rep, ncond, ncodes))
    lat1 = g.last_latents.clone()
    three = g.generate(cond.to(DEV), codes.to(DEV), group=5, **greedy_kw(scale, rep, ncond, ncodes))       # 5 + 5 + 2 steps
    assert one.shape[1] == MAX_NEW
    assert torch.equal(one, three) and torch.equal(lat1, g.last_latents)
    close(g)


# ---- 5. the processors run behind the guidance -------------------------------------------------------------------------------------
PROC_CASE = dict(scale=1.5, rep=2.0, seed=0, stop_bias=8.0, kw=dict(min_new_tokens=6, no_repeat_ngram_size=2))


def test_processors_run_on_the_guided_scores():
    """HF's list is [CFG, repetition, ngram, min_new]: a stop bias that ends the rows early without processors, held off by
    min_new_tokens = 6, with no_repeat_ngram_size = 2"""
    c = PROC_CASE
    r = oracle(gcfg.TINY_MODEL_ARGS, c["seed"], c["scale"], c["rep"], kw=c["kw"], stop_bias=c["stop_bias"])
    screen(r, c["scale"], c["rep"])
    bare = oracle(gcfg.TINY_MODEL_ARGS, c["seed"], c["scale"], c["rep"], stop_bias=c["stop_bias"])
    assert bare["ids"].shape[1] < 6                                   # without the processors every row has stopped before 6 tokens
    stops = [int(np.nonzero(row == EOS)[0][0]) for row in r["ids"]]
    assert min(stops) == 6                                            # ... with them the first stop comes at the first allowed step
    g = make_gpt(gcfg.TINY_MODEL_ARGS, c["seed"], stop_bias=c["stop_bias"])
    cond, codes, ncond, ncodes = inputs(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS))
    ids = g.generate(cond.to(DEV), codes.to(DEV), **greedy_kw(c["scale"], c["rep"], ncond, ncodes, **c["kw"])).cpu().numpy()
    assert np.array_equal(ids, r["ids"])
    off = g.generate(cond.to(DEV), codes.to(DEV), **greedy_kw(c["scale"], c["rep"], ncond, ncodes)).cpu().numpy()
    assert np.array_equal(off, bare["ids"])
    close(g)


# ---- 6. sampling --------------------------------------------------------------------------------------------------------------------
def test_guided_sampling_draws_inside_the_top_k():
    scale, seed, K, temp = 1.5, 0, 15, 0.75
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    g = make_gpt(gcfg.TINY_MODEL_ARGS, seed)
    cond, codes, ncond, ncodes = inputs(dims)
    kw = dict(do_sample=True, top_k=K, temperature=temp, guidance_scale=scale, negative_cond_latents=ncond.to(DEV),
              negative_text_inputs=ncodes.to(DEV))
    a = g.generate(cond.to(DEV), codes.to(DEV), seed=3, **kw).cpu()
    b = g.generate(cond.to(DEV), codes.to(DEV), seed=3, **kw).cpu()
    c = g.generate(cond.to(DEV), codes.to(DEV), seed=4, **kw).cpu()
    assert torch.equal(a, b)
    assert a.shape != c.shape or not torch.equal(a, c)
    # teacher-forced on the device's own tokens: every sampled token lies inside the oracle's top K of the processed guided scores (the
    # scores TopK reads: behind the guidance and the temperature), up to the screen's width at the K-th place.  No step is excluded.
    ora = CF.BO.OracleGpt(synth.make_weights(seed, synth.gpt_weight_spec(dims)), dims)
    r = CF.guided(ora, cond, codes, ncond, ncodes, scale, rep=1.0, sampling=dict(temperature=temp, top_k=0), forced=a)
    slack = (2 * scale - 1) * 2e-3
    live = torch.ones(a.shape[0], dtype=torch.bool)
    worst = np.inf
    for t, s in enumerate(r["scores"]):
        kth = torch.topk(s, K, dim=-1)[0][:, -1]
        mine = s.gather(1, a[:, t:t + 1]).squeeze(1)
        worst = min(worst, float((mine - kth)[live].min()))
        assert bool(((mine >= kth - slack) | ~live).all()), (t, mine, kth)
        live = live & (a[:, t] != EOS)
    print(f"smallest (sampled score - K-th score) {worst:.3e} (slack {slack:.1e})")
    close(g)


# ---- 7. warm path -------------------------------------------------------------------------------------------------------------------
def tiny_model(max_slots=8):
    from genvc_amd.inference.model_init import model_init_synthetic
    m = model_init_synthetic(gcfg.default_config(tiny=True), seed=1, device=DEV, max_slots=max_slots)[0]
    m.gpt.max_gen_mel_tokens = 30
    return m


def test_guided_call_after_warmup_neither_allocates_nor_captures():
    m = tiny_model()
    src = synth.uniform(402, "src_wav", (1, 16000), 0.3).to(DEV)
    ref = synth.uniform(100, "ref_wav", (1, 24000 * 3), 0.3).to(DEV)
    cond = m.get_gpt_cond_latents(ref, 24000)
    m.warmup(seg_len=1.0, streams=1, ref_seconds=3.0, max_new_tokens=30, guidance=True)
    base = m.gpt.engine.lazy_inits()
    wav = m.inference(src, cond, guidance_scale=1.5, generate_kwargs={"seed": 4})
    torch.cuda.synchronize()
    assert m.gpt.engine.lazy_inits() == base
    assert wav.shape[-1] > 0 and wav.shape[-1] % 1024 == 0


# ---- 8. the harness -----------------------------------------------------------------------------------------------------------------
def test_synthesize_utt_with_guidance():
    from genvc_amd.inference.inference_utils import synthesize_utt
    m = tiny_model()
    src = synth.uniform(402, "src_wav", (1, 16000 * 2), 0.3).to(DEV)
    ref = synth.uniform(100, "ref_wav", (1, 24000 * 3), 0.3).to(DEV)
    kw = {"seed": 4}
    plain = synthesize_utt(m, src, ref, seg_len=1.0, generate_kwargs=kw)
    guided = synthesize_utt(m, src, ref, seg_len=1.0, generate_kwargs=kw, guidance_scale=1.5)
    assert guided.ndim == 1 and guided.numel() > 0 and guided.numel() % 1024 == 0 and bool(torch.isfinite(guided).all())
    assert guided.shape != plain.shape or not torch.equal(guided, plain)
    # the default negative reference is the source utterance itself
    explicit = synthesize_utt(m, src, ref, seg_len=1.0, generate_kwargs=kw, guidance_scale=1.5,
                              negative_ref_audio=(src, m.content_sample_rate))
    assert torch.equal(guided, explicit)
    # another negative speaker gives another conversion
    other = synthesize_utt(m, src, ref, seg_len=1.0, generate_kwargs=kw, guidance_scale=1.5,
                           negative_ref_audio=(synth.uniform(101, "ref_wav", (1, 24000 * 2), 0.3).to(DEV), 24000))
    assert other.shape != guided.shape or not torch.equal(other, guided)
    # guidance_scale = 1 is the call without the kwarg, bit for bit
    one = synthesize_utt(m, src, ref, seg_len=1.0, generate_kwargs=kw, guidance_scale=1.0)
    assert torch.equal(one, plain)
