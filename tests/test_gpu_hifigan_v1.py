"""GPU: the HiFi-GAN generator with ResBlock1 (resblock_type "1") against the reference fixture (tests/golden/hifigan_v1.npz) and the
oracle restatement (tests/hifigan_v1_oracle.py, pinned to the reference class by scripts/make_hifigan_v1_golden.py).

Tolerance: the rule of tests/test_gpu_vocoder_eval.py, |device - reference| <= 8 x floor.  A floor is max(max|fp32 - fp64| of the
reference (fixture) or of the oracle (every other shape), 2^-24 max|wav|): what separates two correct fp32 evaluations."""
import numpy as np
import pytest
import torch

import hifigan_v1_oracle as HO
from genvc_amd import config as gcfg
from genvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 8.0


def bound(cfg, max_batch=2, max_frames=64, seed=HO.SEED):
    from genvc_amd.layers.hifigan import HiFiGAN
    m = HiFiGAN(cfg["input_feat_dim"], cfg["upsample_initial_channel"], cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"],
                cfg["upsample_rates"], cfg["upsample_kernel_sizes"], resblock_type=cfg["resblock_type"])
    w = HO.weights(cfg, seed)
    m.load_state_dict(w, strict=True)
    m.to(DEV)
    return m.bind(max_batch=max_batch, max_frames=max_frames), w


def check(label, got, want, floor):
    want = torch.as_tensor(want)
    assert tuple(got.shape) == tuple(want.shape), (label, got.shape, want.shape)
    err = float((got.detach().cpu().double() - want.double()).abs().max())
    print(f"{label}: |device - reference| {err:.3e} = {err / floor:.2f} floors (floor {floor:.3e})")
    assert err <= MARGIN * floor, f"{label}: {err / floor:.2f} floors (floor {floor:.3e}), more than {MARGIN:g}"


@pytest.mark.parametrize("cfg,tags", [(HO.CFG_A, ("a1", "a2")), (HO.CFG_B, ("b1", "b2"))], ids=["widths_128_64", "width_32"])
def test_resblock1_matches_reference_fixture_on_the_small_conv_path(gold, cfg, tags):
    """kernels 3 / 7 / 11, dilations 1 / 3 / 5 at the three widths of the one-round-trip conv kernel: six launches per stage, the
    11-tap instantiations, planes ping-ponging through the second set"""
    g = gold("hifigan_v1")
    m, _ = bound(cfg)
    assert m._engine.resblock_type == 1 and m._engine.lds_stages == len(cfg["upsample_rates"])
    for tag, c, B, T in HO.CASES:
        if tag in tags:
            x = HO.frames(HO.SEED, B, T, cfg["input_feat_dim"]).to(DEV)
            check(f"{tag} B={B} T={T}", m(x), g[f"{tag}_wav"], float(g[f"floor_{tag}"]))
    # head + conv_pre + per stage (upsampling + 6) + conv_post, one straight chain in one graph
    assert m._engine.graph_nodes == 3 + 7 * len(cfg["upsample_rates"])


@pytest.mark.parametrize("cfg", [HO.v1_cfg(256, [2, 2], kernels=[3, 11]), HO.v1_cfg(64, [2], kernels=[3, 11]), HO.v1_cfg(32, [2])],
                         ids=["two_kernels_128_64", "two_kernels_32", "width_16"])
def test_resblock1_launch_per_conv_path_matches_oracle(cfg):
    """what the one-round-trip kernel does not take (n_kernels != 3, a width outside 32 / 64 / 128): t = convs1[m](lrelu(x)),
    x = x + convs2[m](lrelu(t)) as one tiled-GEMM launch per conv, the running sum over blocks and the 1 / n_kernels in the last epilogue"""
    m, w = bound(cfg)
    assert m._engine.lds_stages == 0
    for B, T in ((1, 5), (2, 33)):
        x = HO.frames(HO.SEED, B, T, cfg["input_feat_dim"])
        want, fl = HO.reference(w, cfg, x)
        check(f"B={B} T={T}", m(x.to(DEV)), want, fl)


def test_resblock1_small_conv_switch_takes_the_launch_per_conv_path(monkeypatch):
    """GVC_VOCODER_SMALL_CONV=0: the same generator, every conv on the tiled GEMM"""
    monkeypatch.setenv("GVC_VOCODER_SMALL_CONV", "0")
    m, w = bound(HO.CFG_A)
    assert m._engine.lds_stages == 0
    x = HO.frames(HO.SEED, 2, 33, 64)
    want, fl = HO.reference(w, HO.CFG_A, x)
    check("SMALL_CONV=0 B=2 T=33", m(x.to(DEV)), want, fl)


def test_resblock1_forward_latents_matches_oracle():
    cfg = HO.CFG_A
    m, w = bound(cfg)
    lat = synth.uniform(HO.SEED, "lat_2_9", (2, 9, cfg["input_feat_dim"]), 1.0)
    want, fl = HO.reference(w, cfg, lat, fn=HO.vocode_latents, scale=4)
    check("forward_latents scale 4", m.forward_latents(lat.to(DEV), 4), want, fl)


def test_resblock1_windowed_long_input_matches_single_pass():
    """buffers as small as window_overlap allows, an input about three windows long: every kept sample sees its whole (ResBlock1)
    receptive field, so the stitched output is the oracle's single pass"""
    cfg = HO.CFG_B
    from genvc_amd.layers.hifigan import HiFiGAN
    probe = HiFiGAN(cfg["input_feat_dim"], cfg["upsample_initial_channel"], cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"],
                    cfg["upsample_rates"], cfg["upsample_kernel_sizes"], resblock_type="1")
    ov = probe.window_overlap
    assert ov >= probe.receptive_frames()
    cap = 2 * ov + 16                                  # forward needs more than 2 * overlap + 8 frames of buffer
    m, w = bound(cfg, max_batch=1, max_frames=cap)
    T = 3 * cap + 5
    x = HO.frames(HO.SEED, 1, T, cfg["input_feat_dim"], "long")
    want, fl = HO.reference(w, cfg, x)
    check(f"windows of {cap} frames (overlap {ov}) over {T}", m(x.to(DEV)), want, fl)


def test_resblock1_results_are_bit_stable_across_shapes_without_sync():
    """shape a, shape b, shape a again, enqueued with no host sync in between: the padding rows are re-zeroed on every geometry change
    and the ping-pong planes carry nothing over, so the first and the third result are bit-identical, and b, computed between them,
    is bit-identical to what a fresh engine that has seen nothing else computes for it (and within floors of the oracle)"""
    cfg = HO.CFG_A
    m, w = bound(cfg)
    xa = HO.frames(HO.SEED, 1, 5, cfg["input_feat_dim"]).to(DEV)
    xb = HO.frames(HO.SEED, 2, 33, cfg["input_feat_dim"]).to(DEV)
    torch.cuda.synchronize()
    a1 = m(xa)
    b = m(xb)
    a2 = m(xa)
    torch.cuda.synchronize()
    assert torch.equal(a1, a2)
    assert not torch.equal(b[:1, :, :a1.shape[-1]], a1)
    fresh, _ = bound(cfg)
    b_alone = fresh(xb)
    torch.cuda.synchronize()
    assert torch.equal(b, b_alone), "b was changed by the calls around it"
    assert torch.equal(fresh(xa), a1)                  # and a after b on the fresh engine: the same bits again
    want, fl = HO.reference(w, cfg, xb.cpu())
    check("b between two a calls", b, want, fl)


def test_resblock1_conversion_vocodes_the_devices_own_latents():
    """model_init_synthetic with resblock_type "1" on the tiny config, one short non-streaming conversion: the waveform is the oracle
    vocoder applied to what the device fed its own vocoder"""
    from genvc_amd.inference.model_init import model_init_synthetic
    cfg = gcfg.default_config(tiny=True, resblock_type="1")
    model, _ = model_init_synthetic(cfg, seed=1, device=DEV)
    assert model.hifigan.cfg["resblock_type"] == "1" and model.hifigan._engine.resblock_type == 1
    fed = []
    vocode = model.hifigan.forward
    model.hifigan.forward = lambda x: (fed.append(x.detach().clone()), vocode(x))[1]
    src = synth.synth_audio(5, "src", 16000)
    ref = synth.synth_audio(6, "ref", 72000)
    cond = model.get_gpt_cond_latents(ref.to(DEV), 24000)
    wav = model.inference(src.to(DEV), cond, top_k=1, top_p=0.85, temperature=0.85, repetition_penalty=2.0)
    assert len(fed) == 1 and wav.shape[-1] == fed[0].shape[-1] * 256 and wav.shape[-1] > 0
    w = {k[len("hifigan."):]: v for k, v in model.state_dict().items() if k.startswith("hifigan.")}
    want, fl = HO.reference(w, dict(cfg.vocoder_config), fed[0].cpu())
    check(f"conversion, {fed[0].shape[-1]} frames", wav, want, fl)
