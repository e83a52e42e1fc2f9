"""Host side of TorchMelSpectrogram.invert: the conventions of the CPU oracle (tests/griffinlim_oracle.py) against a direct DFT, the
least-squares inverse against the pseudo-inverse, argument validation before any device access, and the C ABI's three places."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import griffinlim_oracle as GO      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["gvc_gl_create", "gvc_gl_destroy", "gvc_gl_inverse_matrix", "gvc_gl_inverse_mel", "gvc_gl_init_angles", "gvc_gl_run",
           "gvc_gl_launches"]


def direct_istft(spec, n_fft, hop, win):
    """inverse real DFT by the O(N^2) sum (the imaginary parts of bin 0 and of the Nyquist bin do not enter), periodic Hann centred in
    the frame, overlap-add, division by the summed squared windows, n_fft / 2 trimmed from both ends; float64 numpy"""
    B, n_freq, F = spec.shape
    n = np.arange(n_fft)
    k = np.arange(n_freq)
    ang = 2.0 * np.pi * np.outer(n, k) / n_fft
    wgt = np.where((k == 0) | (k == n_fft // 2), 1.0, 2.0)
    w = np.zeros(n_fft)
    off = (n_fft - win) // 2
    w[off:off + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    total = n_fft + hop * (F - 1)
    out = np.zeros((B, hop * (F - 1)))
    for b in range(B):
        y, env = np.zeros(total), np.zeros(total)
        for t in range(F):
            X = spec[b, :, t]
            x = (np.cos(ang) @ (wgt * X.real) - np.sin(ang) @ (wgt * X.imag)) / n_fft
            y[t * hop:t * hop + n_fft] += x * w
            env[t * hop:t * hop + n_fft] += w * w
        out[b] = (y / np.where(env > 0, env, 1.0))[n_fft // 2:n_fft // 2 + hop * (F - 1)]
    return out


@pytest.mark.parametrize("n_fft,win,hop,F,B", [GO.SHAPES[0], GO.SHAPES[3]])
def test_oracle_istft_conventions(n_fft, win, hop, F, B):
    """the F = 2 shapes: every kept sample is covered by fewer than win / hop frames, so the envelope and the trim both matter"""
    S = GO.make_spectrogram(11, B, n_fft // 2 + 1, F).double()
    spec = (S * GO.random_angles(12, B, n_fft // 2 + 1, F)).to(torch.complex128)
    got = GO.istft(spec, n_fft, hop, win).numpy()
    want = direct_istft(spec.numpy(), n_fft, hop, win)
    assert got.shape == want.shape == (B, hop * (F - 1))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # n_iter = 0 of the loop is that istft
    a = GO.random_angles(12, B, n_fft // 2 + 1, F)
    assert torch.equal(GO.griffinlim(S, a, 0, n_fft, hop, win, dtype=torch.float64), GO.istft(S * a, n_fft, hop, win))


@pytest.mark.parametrize("cfg", GO.DVAE_MELS, ids=["24000", "22050"])
def test_gels_is_the_pseudo_inverse(cfg):
    fb = GO.filterbank(cfg["n_fft"], cfg["sample_rate"], cfg["f_min"], cfg["f_max"], cfg["n_mels"], torch.float64)
    assert int(torch.linalg.matrix_rank(fb)) == cfg["n_mels"]
    eye = torch.eye(cfg["n_mels"], dtype=torch.float64)
    gels = torch.linalg.lstsq(fb.T[None], eye[None], driver="gels").solution[0]
    pinv = torch.linalg.pinv(fb.T)
    assert float((gels - pinv).abs().max()) <= 1e-11 * float(pinv.abs().max())
    # and the closed form the library builds: fb (fb^T fb)^-1
    closed = fb @ torch.linalg.inv(fb.T @ fb)
    assert float((closed - pinv).abs().max()) <= 1e-11 * float(pinv.abs().max())


def test_invert_validates_before_the_device():
    from genvc_amd.utils import TorchMelSpectrogram
    tm = TorchMelSpectrogram()
    ok = torch.zeros(1, 80, 4)
    with pytest.raises(ValueError, match="2 frames"):
        tm.invert(torch.zeros(1, 80, 1))
    with pytest.raises(ValueError, match="n_mels=80"):
        tm.invert(torch.zeros(1, 100, 4))
    with pytest.raises(ValueError, match="n_iter"):
        tm.invert(ok, n_iter=-1)
    for m in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="momentum"):
            tm.invert(ok, momentum=m)
    with pytest.raises(ValueError, match="init_angles"):
        tm.invert(ok, init_angles=torch.zeros(1, 513, 3, dtype=torch.complex64))          # wrong shape
    with pytest.raises(ValueError, match="init_angles"):
        tm.invert(ok, init_angles=torch.zeros(1, 513, 4, dtype=torch.complex128))         # wrong dtype
    with pytest.raises(ValueError, match="init_angles"):
        tm.invert(ok, init_angles=torch.zeros(1, 513, 4, 2))                              # real pairs are not complex64
    with pytest.raises(ValueError, match="mel must be"):
        tm.invert(torch.zeros(80, 4))
    assert tm._gl_engine is None                                                          # nothing was created on the way


def test_engine_creation_refusals():
    """creation checks run on the host, before any device call: unsupported configurations and a filterbank without an inverse"""
    from genvc_amd.engine import GriffinLimEngine
    for kw, msg in ((dict(n_fft=4096, win=1024), "n_fft 4096"), (dict(n_fft=256, win=256, hop=64), "n_fft 256"),
                    (dict(n_fft=1000, win=1000, hop=250), "n_fft 1000"), (dict(n_fft=512, win=1024), "win 1024"),
                    (dict(hop=300), "hop 300"), (dict(hop=1024), "hop 1024")):
        with pytest.raises(ValueError, match=msg):
            GriffinLimEngine(**kw)
    # 200 filters on 257 bins: the lowest filters fall between two bins
    with pytest.raises(ValueError, match=r"mel filter \d+ of 200 has no frequency bin"):
        GriffinLimEngine(n_fft=512, win=512, hop=128, n_mels=200, sample_rate=24000)
    # 200 filters on 1025 bins: every filter has a bin, but the narrow ones are not independent
    with pytest.raises(ValueError, match=r"mel filter \d+ of 200 is not independent"):
        GriffinLimEngine(n_fft=2048, win=1024, hop=256, n_mels=200, sample_rate=24000)


def test_new_symbols_declared_and_exported():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    assert re.search(r"typedef struct gvc_gl_options \{[^}]*n_fft, hop, win, sample_rate, n_mels;[^}]*max_batch, max_frames;[^}]*"
                     r"float f_min, f_max;", hdr)
    assert [n for n, _ in _lib.GlOptions._fields_] == ["n_fft", "hop", "win", "sample_rate", "n_mels", "max_batch", "max_frames", "f_min",
                                                       "f_max"]
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s


def test_audition_codes_needs_the_acoustic_dvae():
    from genvc_amd import config as gcfg
    from genvc_amd.inference.model_init import GenVCModel
    plain = GenVCModel(gcfg.default_config(tiny=True))
    with pytest.raises(NotImplementedError, match="acoustic_dvae_config"):
        plain.audition_codes(torch.zeros(1, 4, dtype=torch.long))


def test_audition_codes_is_invert_of_decode():
    """host wiring: the decoded mel (the first of decode's two outputs) goes to the DVAE extractor's invert with n_iter and seed"""
    from genvc_amd import config as gcfg
    from genvc_amd.inference.model_init import GenVCModel
    m = GenVCModel(gcfg.default_config(tiny=True, with_acoustic=True))
    seen = {}

    class Dvae(torch.nn.Module):
        def decode(self, codes):
            seen["codes"] = codes
            return torch.full((codes.shape[0], 80, 4 * codes.shape[1]), 0.5), "pre"

    class Mel(torch.nn.Module):
        def invert(self, mel, **kw):
            seen["mel"], seen["kw"] = mel, kw
            return "wav"

    m.acoustic_dvae, m.torch_mel_spectrogram_dvae = Dvae(), Mel()
    codes = torch.zeros(2, 3, dtype=torch.long)
    assert m.audition_codes(codes, n_iter=5, seed=9) == "wav"
    assert seen["codes"] is codes and seen["mel"].shape == (2, 80, 12) and seen["kw"] == dict(n_iter=5, seed=9)
    assert math.isclose(float(seen["mel"][0, 0, 0]), 0.5)
