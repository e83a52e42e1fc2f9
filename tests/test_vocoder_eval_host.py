"""CPU: the vocoder-evaluation oracle against the reference fixture (tests/golden/vocoder_eval.npz), the state-dict names, both weight
folds, the closed-form properties of the restated Slaney filterbank, the refusals of evaluate_vocoder and the new C symbols."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocoder_eval_oracle as VO      # noqa: E402
from genvc_amd import config as gcfg  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gvc_disc_create", "gvc_disc_destroy", "gvc_disc_bind_weight", "gvc_disc_missing_weights", "gvc_disc_folded_weight",
           "gvc_disc_arena_floats", "gvc_disc_set_arena", "gvc_disc_layers", "gvc_disc_layer", "gvc_disc_forward", "gvc_disc_time_layer", "gvc_l1_mean",
           "gvc_mel_create_ex", "gvc_mel_frames"]


def oracle_quantities(outs):
    d_r, d_g, f_r, f_g = outs
    n = lambda t: t.detach().double().numpy()                      # noqa: E731
    q = {}
    for i in range(len(d_r)):
        q[f"dr{i}"], q[f"dg{i}"] = n(d_r[i]), n(d_g[i])
        for l in range(len(f_r[i])):
            q[f"fr{i}_{l}"], q[f"fg{i}_{l}"] = n(VO.subsample(f_r[i][l])), n(VO.subsample(f_g[i][l]))
    q["fmean"] = np.array([[float(v) for v in row] for row in VO.feature_means(f_r, f_g)])
    loss, rl, gl = VO.discriminator_criterion(d_r, d_g)
    gen, genl = VO.generator_criterion(d_g)
    q["disc"], q["rl"], q["gl"] = n(loss), np.array(rl), np.array(gl)
    q["gen"], q["genl"], q["feat"] = n(gen), np.array([float(v) for v in genl]), n(VO.feature_criterion(f_r, f_g))
    return q


@pytest.mark.parametrize("tag,B,T,mult", VO.CASES)
@torch.inference_mode()
def test_oracle_reproduces_the_reference_fixture(gold, tag, B, T, mult):
    g = gold("vocoder_eval")
    y, y_hat = VO.wav_pair(int(g["seed"]), B, T)
    cfg = VO.mpd_cfg(mult)
    for D in ("msd", "mpd"):
        w = VO.msd_weights() if D == "msd" else VO.mpd_weights(cfg)
        q = oracle_quantities(VO.msd(w, y, y_hat) if D == "msd" else VO.mpd(w, cfg["mpd_reshapes"], y, y_hat))
        pre = f"{tag}_{D}_"
        names = [k[len(pre):] for k in g.files if k.startswith(pre) and k[len(pre)] != "w" and not k.endswith("keys")]
        assert sorted(names) == sorted(q)
        for k in names:
            err, fl = float(np.abs(q[k] - g[pre + k]).max()), float(np.min(g["floor_" + pre + k]))
            assert q[k].shape == g[pre + k].shape and err <= fl, (tag, D, k, err, fl)
        # O(1) logits: the squared losses are informative
        top = max(float(np.abs(q[f"dr{i}"]).max()) for i in range(len(cfg["mpd_reshapes"]) if D == "mpd" else 3))
        assert 0.05 < top < 20.0, top


@torch.inference_mode()
def test_mel_oracle_reproduces_the_reference_fixture(gold):
    g = gold("vocoder_eval")
    y, y_hat = VO.wav_pair(int(g["seed"]), 2, 4096)
    feat = VO.extract_mel_features(y.reshape(2, 4096))
    assert float(np.abs(feat[0].numpy() - g["mel_feat"]).max()) <= float(g["floor_mel_feat"])
    assert abs(float(VO.mel_criterion(y, y_hat)) - float(g["mel_loss"])) <= float(g["floor_mel_loss"])


def test_state_dict_names_and_strict_load(gold):
    from genvc_amd.layers.hifigan import MultiPeriodDiscriminator, MultiScaleDiscriminator
    g = gold("vocoder_eval")
    msd = MultiScaleDiscriminator()
    assert list(msd.state_dict().keys()) == [str(k) for k in g["a_msd_keys"]]
    msd.load_state_dict(VO.msd_weights(), strict=True)
    for tag, _, _, mult in VO.CASES:
        cfg = VO.mpd_cfg(mult)
        mpd = MultiPeriodDiscriminator(cfg["mpd_reshapes"], mult, False)
        assert list(mpd.state_dict().keys()) == [str(k) for k in g[f"{tag}_mpd_keys"]]
        mpd.load_state_dict(VO.mpd_weights(cfg), strict=True)
    sn = MultiPeriodDiscriminator([2, 3], 0.25, True)
    sn.load_state_dict(VO.mpd_weights(VO.mpd_cfg(0.25, (2, 3), True)), strict=True)
    assert "discriminators.1.convs.0.weight_orig" in sn.state_dict() and "discriminators.1.convs.0.weight_u" in dict(sn.named_buffers())
    v = gcfg.default_config().vocoder_config
    assert v.mpd_reshapes == [2, 3, 5, 7, 11] and v.mpd_discriminator_channel_mult_factor == 1 and v.mpd_use_spectral_norm is False
    assert (v.sample_rate, v.fft_size, v.num_mels, v.mel_fmin, v.mel_fmax, v.win_length, v.hop_length) == (24000, 1024, 100, 0, 12000, 1024, 256)


def test_weight_folds_agree_with_the_fixture(gold):
    g = gold("vocoder_eval")
    seen = set()
    for tag, _, _, mult in VO.CASES:
        for D in ("msd", "mpd"):
            w = VO.msd_weights() if D == "msd" else VO.mpd_weights(VO.mpd_cfg(mult))
            pre = f"{tag}_{D}_w"
            for k in g.files:
                if k.startswith(pre):
                    i, l = (int(v) for v in k[len(pre):].split("_"))
                    n_convs = 7 if D == "msd" else 5
                    name = f"discriminators.{i}." + ("conv_post" if l == n_convs else f"convs.{l}")
                    seen.add("sn" if name + ".weight_orig" in w else "wn")
                    assert np.array_equal(VO.folded(w, name).reshape(-1)[:64].numpy(), g[k]), k
    assert seen == {"sn", "wn"}
    # the folds by their definitions: unit-g weight norm has unit rows; sigma scales the spectral fold
    v, gg = torch.randn(6, 4, 5, dtype=torch.float64), torch.rand(6, 1, 1, dtype=torch.float64) + 0.5
    assert torch.allclose(VO.fold_weight_norm(gg, v).reshape(6, -1).norm(dim=1), gg.reshape(6))
    o, u, s = torch.randn(6, 4, 5, dtype=torch.float64), torch.randn(6, dtype=torch.float64), torch.randn(20, dtype=torch.float64)
    f = VO.fold_spectral_norm(o, u, s)
    assert torch.allclose(torch.dot(u, f.reshape(6, -1) @ s), torch.ones((), dtype=torch.float64))
    # the synthetic spectral vectors keep sigma well away from zero (near 1 / 1.6)
    w = VO.msd_weights()
    for j in (0, 3, 6):
        n = f"discriminators.0.convs.{j}"
        sigma = float(torch.dot(w[n + ".weight_u"], w[n + ".weight_orig"].reshape(w[n + ".weight_u"].numel(), -1) @ w[n + ".weight_v"]))
        assert 0.3 < sigma < 1.2, (n, sigma)


def test_slaney_filterbank_closed_form_properties():
    sr, n_fft, n_mels, fmin, fmax = 24000, 1024, 100, 0, 12000
    fb = VO.slaney_filterbank(sr, n_fft, n_mels, fmin, fmax).astype(np.float64)
    assert fb.shape == (100, 513) and fb.dtype == np.float64 and (fb >= 0).all()
    c = VO.mel_centres(n_mels, fmin, fmax)
    freqs = np.linspace(0, sr / 2, 513)
    mels = VO.hz_to_mel(c)
    assert np.allclose(np.diff(mels), mels[1] - mels[0])                      # equally spaced on the mel scale
    assert np.allclose(VO.mel_to_hz(VO.hz_to_mel(freqs)), freqs)
    # linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (a factor 6.4 every 27 mels), continuous at 1 kHz
    assert np.allclose(VO.hz_to_mel([200.0, 500.0, 1000.0]), [3.0, 7.5, 15.0])
    assert np.isclose(VO.hz_to_mel(6400.0) - VO.hz_to_mel(1000.0), 27.0)
    assert np.isclose(VO.hz_to_mel(1000.0 + 1e-9), 15.0)
    below = c[c < 1000.0]
    assert np.allclose(np.diff(below), below[1] - below[0])
    above = c[c > 1000.0]
    assert np.allclose(above[1:] / above[:-1], above[1] / above[0])
    for i in range(n_mels):
        lo, mid, hi = c[i], c[i + 1], c[i + 2]
        peak = 2.0 / (hi - lo)                                               # Slaney area normalisation: a triangle of unit area in Hz
        # the triangle evaluated at every bin: rises lo -> mid, falls mid -> hi, zero outside
        want = np.maximum(0.0, np.minimum((freqs - lo) / (mid - lo), (hi - freqs) / (hi - mid))) * peak
        assert np.allclose(fb[i], want, rtol=1e-6, atol=1e-12), i
        assert fb[i].max() <= peak * (1 + 1e-6)
        inside = (freqs > lo) & (freqs < hi)
        assert (fb[i][~inside] == 0).all()
        if inside.sum() >= 8:                                                # wide bands: the sampled area approaches 1
            assert abs(fb[i].sum() * (freqs[1] - freqs[0]) - 1.0) < 0.05, i
        k = int(np.argmax(fb[i]))
        if inside.any():
            assert abs(freqs[k] - mid) <= freqs[1] - freqs[0]                # peaks at the bin nearest its centre


def test_evaluate_vocoder_rejects_unserved_discriminators_and_training_mode():
    from genvc_amd.inference.model_init import GenVCModel
    from genvc_amd.layers import hifigan as H
    model = GenVCModel(gcfg.default_config(tiny=True, with_acoustic=True))
    for key in ("MSTFT", "MSCQT"):
        with pytest.raises(NotImplementedError, match=key):
            model.evaluate_vocoder({}, discriminators=("MSD", key))
    assert model._vocoder_discriminator("MPD").d_mult == 0.25 and not model._vocoder_discriminator("MSD").training
    for cls in (H.MultiScaleSTFTDiscriminator, H.MultiScaleSubbandCQTDiscriminator):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls()
    d = H.MultiPeriodDiscriminator([2, 3], 0.25, False)
    assert d.training
    with pytest.raises(NotImplementedError, match="eval mode"):
        d(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64))


def test_criteria_fall_back_to_the_reference_arithmetic_on_plain_tensors():
    from genvc_amd.layers import hifigan_loss as HL
    torch.manual_seed(0)
    d_r, d_g = [torch.randn(2, 7), torch.randn(2, 3)], [torch.randn(2, 7), torch.randn(2, 3)]
    f_r = [[torch.randn(2, 4, 7)], [torch.randn(2, 4, 3), torch.randn(2, 1, 3)]]
    f_g = [[torch.randn(2, 4, 7)], [torch.randn(2, 4, 3), torch.randn(2, 1, 3)]]
    loss, rl, gl = HL.discriminator_criterion()(d_r, d_g)
    o_loss, o_rl, o_gl = VO.discriminator_criterion(d_r, d_g)
    assert torch.equal(loss, o_loss) and rl == o_rl and gl == o_gl
    gen, genl = HL.generator_criterion()(d_g)
    o_gen, o_genl = VO.generator_criterion(d_g)
    assert torch.equal(gen, o_gen) and all(torch.equal(a, b) for a, b in zip(genl, o_genl))
    assert torch.equal(HL.feature_criterion()(f_r, f_g), VO.feature_criterion(f_r, f_g))


def test_new_symbols_are_declared_and_exported():
    import subprocess
    from genvc_amd import _lib
    from genvc_amd.build import build
    header = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", build(verbose=False)], capture_output=True, text=True, check=True).stdout
    have = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for s in SYMBOLS:
        assert s in _lib.exported_symbols() and f" {s}(" in header and s in have, s
    assert any(n == "mel_norms_host" for n, _ in _lib.MelOptions._fields_) and _lib.DiscDims._fields_[2][0] == "periods"
