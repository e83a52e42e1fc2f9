"""CPU tests of tests/act_stats.py: every preset reaches its declared regime under the float64 oracle, and the float64 oracle on
the default synthetic weights agrees with the float32 oracle to float32 precision (including the bf16 rounding modes)."""
import pytest
import torch

import act_stats as A
from genvc_amd import config as gcfg
from genvc_amd import synth
from oracle import genvc_oracle as O

MARGS = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2)


def _gpt_case(preset, Tc=13, steps=2, B=1):
    dims = gcfg.gpt_dims(MARGS)
    w = A.gpt_weights(synth.make_weights(3, synth.gpt_weight_spec(dims)), dims, preset)
    d = dims["d_model"]
    cond = A.cond_latents(synth.uniform(7, "cond_latents", (B, 32, d), 1.0), d, preset)
    codes = synth.integers(7, "content_codes", (B, Tc), 256)
    toks = synth.integers(8, "toks", (B, steps), 1024)
    return dims, w, cond, codes, toks


def _run(w, dims, cond, codes, toks):
    emb = O.compute_embeddings(w, dims, cond, codes)[0]
    z, lg, cache = O.gpt_prefill(w, dims, emb)
    outs = [(z, lg)]
    for j in range(1, toks.shape[1] + 1):
        z, lg, cache = O.gpt_decode_step(w, dims, cache, toks[:, j - 1], j)
        outs.append((z, lg))
    return outs


@pytest.mark.parametrize("preset", ["offset", "offset30", "outliers", "peaked", "all"])
def test_gpt_presets_reach_their_regime(preset):
    dims, w, cond, codes, toks = _gpt_case(preset)
    with A.record() as st:
        _run(A.double(w), dims, cond.double(), codes, toks)
    A.check_regime(preset, st, "gpt")


def test_default_weights_stay_tame():
    """the knobs are what moves the statistics: the default weights are far from every regime"""
    dims, w, cond, codes, toks = _gpt_case("default")
    with A.record() as st:
        _run(A.double(w), dims, cond.double(), codes, toks)
    s = A.summary(st)
    assert s["ln_ratio"] < 1.0 and s["max_abs"] < 20.0 and s["spread"] < 20.0, s


@pytest.mark.parametrize("mode", ["fp32", "bf16_kv"])
def test_float64_oracle_agrees_with_float32_on_default_weights(mode):
    dims, w, cond, codes, toks = _gpt_case("default", steps=3)
    if mode != "fp32":
        w = {k: v.to(torch.bfloat16).float() for k, v in w.items()}
        dims = dict(dims, kv_bf16=True)
    o32 = _run(w, dims, cond, codes, toks)
    o64 = _run(A.double(w), dims, cond.double(), codes, toks)
    assert o64[0][1].dtype == torch.float64 and o32[0][1].dtype == torch.float32
    for (z32, l32), (z64, l64) in zip(o32, o64):
        # (bf16_kv: a k / v value can round to the other bf16 neighbour in the two precisions; the act_bf16 mode rounds every
        # activation and drifts by ~1e-2 between them, so it has no float32-precision agreement to assert)
        tol = 2e-5 if mode == "fp32" else 5e-3
        assert A.maxdev(l32, l64) < tol and A.maxdev(z32, z64) < tol, (A.maxdev(l32, l64), A.maxdev(z32, z64))


def test_bf16_rounding_keeps_the_dtype():
    x = torch.tensor([1.0 + 2 ** -9, 3.14159], dtype=torch.float64)
    assert O._bf16(x).dtype == torch.float64
    assert torch.equal(O._bf16(x), x.to(torch.bfloat16).double())
    assert torch.equal(O._bf16(x.float()), x.float().to(torch.bfloat16).float())


def test_perceiver_peaked_preset_reaches_its_regime():
    d = 1024
    w = synth.make_weights(1, synth.perceiver_weight_spec(d, prefix="conditioning_perceiver."))
    mel = synth.uniform(4, "mel", (1, 80, 120), 1.0)
    run = lambda ww: O.perceiver_forward(ww, mel.double().permute(0, 2, 1))
    wp = A.perceiver_weights(w, run)
    with A.record() as st:
        run(A.double(wp))
    A.check_regime("peaked", st, "perceiver")


def test_hubert_peaked_and_dc_reach_their_regime():
    c = gcfg.TINY_HUBERT
    w = synth.make_weights(23, synth.hubert_weight_spec(c))
    wav = synth.synth_audio(41, "dc", 16000)
    run = lambda ww: O.hubert_extract_features(ww, c, wav.double())
    wp = A.hubert_weights(w, c, run)
    with A.record() as st:
        run(A.double(wp))
    A.check_regime("peaked", st, "hubert")
    with A.record() as st:
        O.hubert_extract_features(A.double(w), c, A.dc_audio(wav).double())
    A.check_regime("dc", st, "hubert")
    assert bool((A.dc_audio(wav) != 0).all())                 # a DC input is not padding
