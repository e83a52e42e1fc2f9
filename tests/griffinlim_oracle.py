"""CPU restatement of TorchMelSpectrogram.invert (reference utils.py:164-172): exp(mel * norms), torchaudio 2.3's InverseMelScale
(relu of the least-squares solution, driver "gels") and librosa 0.10's griffinlim (momentum, zero-padded centred STFT, periodic Hann).
torchaudio and librosa are absent here: both are restated from their published algorithms and NOT pinned against the libraries, as the
Slaney filterbank already is (oracle/genvc_oracle.py)."""
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.genvc_oracle import mel_filterbank      # noqa: E402

EPS = float(torch.finfo(torch.float32).tiny)        # librosa.util.tiny of a float32 array

# (n_fft, win, hop, F, B) of the GPU tests: fewer than 4 covering frames; first full overlap and the batch stride; ...; a zero-padded
# window; ...; the smallest FFT
SHAPES = [(1024, 1024, 256, 2, 1), (1024, 1024, 256, 5, 2), (1024, 1024, 256, 9, 1), (2048, 1024, 256, 2, 1), (2048, 1024, 256, 7, 2),
          (512, 512, 128, 3, 1)]
LONG_SHAPES = [(1024, 1024, 256, 9, 1), (2048, 1024, 256, 7, 2)]
# the two DVAE mels: TorchMelSpectrogram's defaults at GenVC's 24 kHz and at the class's own 22050 Hz
DVAE_MELS = [dict(n_fft=1024, hop=256, win=1024, sample_rate=24000, f_min=0.0, f_max=8000.0, n_mels=80),
             dict(n_fft=1024, hop=256, win=1024, sample_rate=22050, f_min=0.0, f_max=8000.0, n_mels=80)]


def filterbank(n_fft, sample_rate, f_min, f_max, n_mels, dtype=torch.float32):
    """[n_freq, n_mels], the filterbank of forward()"""
    return mel_filterbank(n_fft // 2 + 1, f_min, f_max, n_mels, sample_rate, dtype)


def inverse_mel(mel, norms, fb):
    """mel [B,n_mels,F] (normalised log power mel), norms [n_mels] or None, fb [n_freq,n_mels] -> relu(lstsq(fb^T, exp(mel norms)))"""
    dt = fb.dtype
    x = mel.to(dt)
    if norms is not None:
        x = x * norms.to(dt).view(1, -1, 1)
    p = torch.exp(x)
    return torch.relu(torch.linalg.lstsq(fb.transpose(0, 1)[None], p, driver="gels").solution)


def _window(win, like):
    return torch.hann_window(win, periodic=True, dtype=like.real.dtype, device=like.device)


def stft(x, n_fft, hop, win):
    return torch.stft(x, n_fft, hop, win, window=_window(win, x), center=True, pad_mode="constant", normalized=False, onesided=True,
                      return_complex=True)


def istft(spec, n_fft, hop, win):
    return torch.istft(spec, n_fft, hop, win, window=_window(win, spec), center=True, normalized=False, onesided=True,
                       return_complex=False)


def griffinlim(S, init_angles, n_iter, n_fft, hop, win, momentum=0.99, dtype=torch.float32):
    """S [B,n_freq,F] >= 0, init_angles complex [B,n_freq,F] -> wav [B, hop (F - 1)]"""
    cdt = torch.complex64 if dtype == torch.float32 else torch.complex128
    S = S.to(dtype)
    angles = init_angles.to(cdt)
    alpha = momentum / (1 + momentum)
    tprev = None
    for _ in range(n_iter):
        inverse = istft(S * angles, n_fft, hop, win)
        rebuilt = stft(inverse, n_fft, hop, win)
        angles = rebuilt if tprev is None else rebuilt - alpha * tprev
        angles = angles / (angles.abs() + EPS)
        tprev = rebuilt
    return istft(S * angles, n_fft, hop, win)


def spectral_convergence(wav, S, n_fft, hop, win):
    """| |stft(wav)| - S |_F / |S|_F per item, in float64"""
    mag = stft(wav.double(), n_fft, hop, win).abs()
    S = S.double()
    return torch.linalg.norm((mag - S).flatten(1), dim=1) / torch.linalg.norm(S.flatten(1), dim=1)


def make_spectrogram(seed, B, n_freq, F):
    """S = 10 rand^4 with bins 5..8 zero and, where F > 2, frame F // 2 zero"""
    g = torch.Generator().manual_seed(seed)
    S = 10.0 * torch.rand(B, n_freq, F, generator=g, dtype=torch.float64) ** 4
    S[:, 5:9] = 0.0
    if F > 2:
        S[:, :, F // 2] = 0.0
    return S.float()


def random_angles(seed, B, n_freq, F, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    ph = 2.0 * math.pi * torch.rand(B, n_freq, F, generator=g, dtype=torch.float64)
    return torch.polar(torch.ones_like(ph), ph).to(torch.complex64 if dtype == torch.float32 else torch.complex128)


def harmonic_noise_wav(seed, B, T, sample_rate):
    """harmonics of 180 Hz with a decaying spectrum plus a little white noise, peak about 0.5"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64) / sample_rate
    x = sum(math.sin(1.0 + h) / h * torch.sin(2.0 * math.pi * 180.0 * h * t + 0.3 * h) for h in range(1, 20))
    x = 0.25 * x.unsqueeze(0).repeat(B, 1) + 0.01 * torch.randn(B, T, generator=g, dtype=torch.float64)
    return x.float()


def floor_of(a32, a64):
    """the project's floor: what fp32 arithmetic costs the oracle, and never less than half an ulp of the largest entry"""
    a32, a64 = a32.double(), a64.double()
    return max(float((a32 - a64).abs().max()), 2.0 ** -24 * float(a64.abs().max()))
