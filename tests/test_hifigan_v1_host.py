"""CPU: the HiFi-GAN generator with ResBlock1 (resblock_type "1") -- the oracle restatement against the reference fixture
(tests/golden/hifigan_v1.npz, scripts/make_hifigan_v1_golden.py), the module's parameter names, its receptive field and the
constructor's checks.  Nothing here needs a GPU: the module only holds parameters until it is bound."""
import numpy as np
import pytest
import torch

import hifigan_v1_oracle as HO
from genvc_amd import config as gcfg
from genvc_amd import synth
from genvc_amd.layers.hifigan import HiFiGAN


def module(cfg):
    return HiFiGAN(cfg["input_feat_dim"], cfg["upsample_initial_channel"], cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"],
                   cfg["upsample_rates"], cfg["upsample_kernel_sizes"], resblock_type=cfg.get("resblock_type", "2"))


@pytest.mark.parametrize("tag,cfg,B,T", HO.CASES, ids=[c[0] for c in HO.CASES])
def test_oracle_matches_reference_fixture(gold, tag, cfg, B, T):
    """The fixture's floor is at least max|fp32 - fp64| of the reference, and the fp64 oracle is the fp64 reference up to fp64 rounding:
    the fp64 oracle lies within one floor of the stored fp32 waveform wherever this runs.  The fp32 oracle's own rounding depends on
    the host (the generating script asserts it within one floor there); here it gets its own distance from the fp64 oracle on top."""
    g = gold("hifigan_v1")
    assert int(g["seed"]) == HO.SEED
    w, x = HO.weights(cfg), HO.frames(HO.SEED, B, T, cfg["input_feat_dim"])
    o32, o64 = HO.generator(w, cfg, x), HO.generator(w, cfg, x.double())
    ref = g[f"{tag}_wav"].astype(np.float64)
    assert tuple(o32.shape) == ref.shape and o32.dtype == torch.float32 and o64.dtype == torch.float64
    fl = float(g[f"floor_{tag}"])
    e64, e32 = float(np.abs(o64.numpy() - ref).max()), float(np.abs(o32.numpy().astype(np.float64) - ref).max())
    own = float((o32.double() - o64).abs().max())
    print(f"{tag}: |oracle - reference| fp64 {e64:.3e}, fp32 {e32:.3e} (own fp32 error {own:.3e}), floor {fl:.3e}")
    slack = 2.0 ** -40                  # two fp64 evaluations of the same sums (reference, oracle): ~1e-16 apart, far below any floor
    assert e64 <= fl + slack
    assert e32 <= fl + own + slack
    assert 1e-3 <= float(np.abs(ref).max()) <= 0.99                 # neither degenerate nor saturated


@pytest.mark.parametrize("tag,cfg,B,T", HO.CASES[1::2], ids=["a", "b"])
def test_state_dict_names_match_reference(gold, tag, cfg, B, T):
    g = gold("hifigan_v1")
    m = module(cfg)
    sd = m.state_dict()
    assert set(sd) == set(str(k) for k in g[f"{tag}_keys"]) and len(sd) == len(g[f"{tag}_keys"])
    spec = synth.hifigan_weight_spec(cfg)
    assert set(sd) == set(spec) and all(tuple(sd[k].shape) == tuple(spec[k][0]) for k in spec)
    assert "resblocks.2.convs1.2.weight_v" in sd and "resblocks.0.convs2.0.bias" in sd and "resblocks.0.convs.0.bias" not in sd
    m.load_state_dict(HO.weights(cfg), strict=True)


def test_default_block_is_resblock1_like_the_reference():
    """the constructor's default is the reference's ("1"); anything but "1" builds ResBlock2 (layers/hifigan.py:181)"""
    c = HO.CFG_B
    m = HiFiGAN(c["input_feat_dim"], c["upsample_initial_channel"], c["resblock_kernel_sizes"], c["resblock_dilation_sizes"],
                c["upsample_rates"], c["upsample_kernel_sizes"])
    assert m.cfg["resblock_type"] == "1" and hasattr(m.resblocks[0], "convs1")
    for t in ("2", 2, "x"):
        m2 = module(dict(c, resblock_type=t, resblock_dilation_sizes=[[1, 3]] * 3))
        assert m2.cfg["resblock_type"] == "2" and hasattr(m2.resblocks[0], "convs") and not hasattr(m2.resblocks[0], "convs1")
    assert module(dict(c, resblock_type=1)).cfg["resblock_type"] == "1"


def test_dilation_lists_of_the_wrong_length_are_refused():
    c = HO.CFG_B
    with pytest.raises(ValueError):
        module(dict(c, resblock_dilation_sizes=[[1, 3]] * 3))                            # ResBlock1 with two dilations
    with pytest.raises(ValueError):
        module(dict(c, resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5, 7]]))
    with pytest.raises(ValueError):
        module(dict(c, resblock_type="2"))                                               # ResBlock2 with three


def test_receptive_frames_covers_the_measured_field_resblock1():
    """V1 kernels and dilations: receptive_frames() is at least what one changed input frame reaches on the oracle; window_overlap
    follows from it"""
    cfg = HO.CFG_A
    m = module(cfg)
    # per block sum_d ((k - 1) / 2 * d + (k - 1) / 2): k = 11 reaches 5 * (1 + 3 + 5) + 15 = 60 samples at each stage's rate
    want = 3.0 + (2 + 60) / 2.0 + (2 + 60) / 4.0 + 3.0 / 4.0
    assert m.receptive_frames() == want
    got = HO.measured_receptive_frames(HO.weights(cfg), cfg, T=160)
    print(f"ResBlock1 {cfg['upsample_rates']}: measured {got:.2f} frames, receptive_frames() {m.receptive_frames():.2f}")
    assert want - 2.0 <= got <= m.receptive_frames()
    assert m.window_overlap >= m.receptive_frames() + 8 and m.window_overlap % 8 == 0


def test_receptive_frames_of_the_trained_resblock2_config_is_unchanged():
    cfg = dict(gcfg.DEFAULT_VOCODER)
    m = module(cfg)
    assert m.receptive_frames() == 10.65625 and m.window_overlap == 32          # 3 + 53/8 + 53/64 + 49/256 + 3/256
    got = HO.measured_receptive_frames(synth.make_weights(HO.SEED, synth.hifigan_weight_spec(cfg)), cfg, T=40)
    print(f"ResBlock2 trained config: measured {got:.2f} frames, receptive_frames() {m.receptive_frames():.2f}")
    assert got <= m.receptive_frames()


def test_config_and_synthetic_weights_for_resblock1():
    assert gcfg.default_config().vocoder_config.resblock_type == "2"
    v = gcfg.default_config(tiny=True, resblock_type="1").vocoder_config
    assert v.resblock_type == "1" and v.resblock_kernel_sizes == [3, 7, 11] and v.resblock_dilation_sizes == [[1, 3, 5]] * 3
    assert gcfg.DEFAULT_VOCODER["resblock_type"] == "2" and gcfg.DEFAULT_VOCODER["resblock_kernel_sizes"] == [3, 5, 7]
    spec = synth.hifigan_weight_spec(v)
    nb = len(v.upsample_rates) * 3
    assert len(spec) == 3 * (2 + len(v.upsample_rates) + 6 * nb)                 # weight_g, weight_v, bias per conv; 6 convs per block
    # the engine's struct carries the block type and three dilations per kernel
    from genvc_amd import _lib
    d = _lib.HifiganDimsEx()
    assert len(d.res_dilations) == 4 and len(d.res_dilations[0]) == 3 and hasattr(d, "resblock_type")
    assert {"gvc_hifigan_create", "gvc_hifigan_create_ex", "gvc_hifigan_lds_stages"} <= set(_lib.exported_symbols())
