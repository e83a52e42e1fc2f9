"""TorchMelSpectrogram with the reference's signature (/root/reference/utils.py:97-172) on
libgenvc_hip (gvc_mel_forward; invert: gvc_gl_inverse_mel, gvc_gl_run)."""
import os

import numpy as np
import torch
from torch import nn

from .engine import GriffinLimEngine, MelEngine

DEFAULT_MEL_NORM_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "mel_stats.npy")


def load_mel_norms(path):
    """mel_stats.pth of the reference (a float32[80] tensor) or the .npy copy shipped in assets/."""
    if path is None:
        return None
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32)
    return torch.load(path, map_location="cpu").numpy().astype(np.float32)


class TorchMelSpectrogram(nn.Module):
    def __init__(self, filter_length=1024, hop_length=256, win_length=1024, n_mel_channels=80, mel_fmin=0,
                 mel_fmax=8000, sampling_rate=22050, normalize=False, mel_norm_file=DEFAULT_MEL_NORM_FILE):
        super().__init__()
        if normalize:
            raise NotImplementedError("normalized=True STFT is not used by GenVC (hifigan_trainer.py:105-115)")
        norms = load_mel_norms(mel_norm_file)
        self.mel_norms = None if norms is None else torch.from_numpy(norms)
        self.args = dict(n_fft=filter_length, hop=hop_length, win=win_length, sample_rate=sampling_rate,
                         f_min=float(mel_fmin), f_max=float(mel_fmax), n_mels=n_mel_channels)
        self._engine = None
        self._gl_engine = None

    @torch.inference_mode()
    def forward(self, inp, frames_major=False):
        if inp.dim() == 3:
            inp = inp.squeeze(1)
        assert inp.dim() == 2
        if self._engine is None:
            norms = np.ones(self.args["n_mels"], np.float32) if self.mel_norms is None else self.mel_norms.numpy()
            self._engine = MelEngine(norms, **self.args)
        return self._engine.forward(inp.to(torch.float32).contiguous(), frames_major=frames_major)

    def bind_invert(self, max_batch=1, max_frames=1024):
        """(re-)create the inversion engine with room for `max_batch` items of `max_frames` frames"""
        if self._gl_engine is not None:
            self._gl_engine.close()
        self._gl_engine = GriffinLimEngine(None if self.mel_norms is None else self.mel_norms.numpy(), max_batch=max_batch,
                                           max_frames=max_frames, **self.args)
        return self

    def _check_invert(self, mel, n_iter, momentum, init_angles):
        if not torch.is_tensor(mel) or mel.dim() != 3 or not mel.is_floating_point():
            raise ValueError(f"invert: mel must be a floating-point tensor [B, n_mels, F], got {tuple(getattr(mel, 'shape', ()))}")
        B, n_mels, F = mel.shape
        if n_mels != self.args["n_mels"]:
            raise ValueError(f"invert: mel has {n_mels} channels, this extractor has n_mels={self.args['n_mels']}")
        if B < 1 or F < 2:
            raise ValueError(f"invert: {F} frames of {B} items: at least 2 frames are needed (the waveform has hop * (F - 1) samples)")
        if int(n_iter) != n_iter or n_iter < 0:
            raise ValueError(f"invert: n_iter={n_iter!r} must be an integer >= 0")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"invert: momentum={momentum!r} must lie in [0, 1)")
        if init_angles is not None:
            want = (B, self.args["n_fft"] // 2 + 1, F)
            if not torch.is_tensor(init_angles) or init_angles.dtype != torch.complex64 or tuple(init_angles.shape) != want:
                raise ValueError(f"invert: init_angles must be a complex64 tensor {want}, got "
                                 f"{getattr(init_angles, 'dtype', type(init_angles))} {tuple(getattr(init_angles, 'shape', ()))}")

    @torch.inference_mode()
    def invert(self, mel, n_iter=64, momentum=0.99, seed=0, init_angles=None):
        """mel [B,n_mels,F] (the output of forward or of DiscreteVAE.decode: a normalised log power mel) -> device tensor
        [B, hop (F - 1)]; `.squeeze().cpu().numpy()` of a one-item call has the reference's return shape (utils.py:164-172).

        exp(mel * norms), torchaudio's InverseMelScale (relu of the minimum-norm least-squares solution), then `n_iter` iterations of
        librosa.griffinlim (momentum, zero-padded centred STFT).  As in the reference, the inverted POWER spectrogram is handed to
        Griffin-Lim where a magnitude belongs; that behaviour is kept.  The reference starts from unseeded NumPy phases, so only the
        algorithm can be matched, not its draws: here the start is `init_angles` (complex64 [B, n_fft / 2 + 1, F]) or, without it, unit
        phasors from the counter-based generator keyed by (seed, item, bin, frame).  Arguments are validated before any device access."""
        self._check_invert(mel, n_iter, momentum, init_angles)
        B, _, F = mel.shape
        eng = self._gl_engine
        if eng is None or B > eng.max_batch or F > eng.max_frames:
            self.bind_invert(max_batch=max(B, eng.max_batch if eng else 1), max_frames=max(F, eng.max_frames if eng else 1024))
            eng = self._gl_engine
        S = eng.inverse_mel(mel.to("cuda" if not mel.is_cuda else mel.device, torch.float32).contiguous())
        if init_angles is not None:
            init_angles = init_angles.to(S.device)
        return eng.griffinlim(S, init_angles=init_angles, seed=seed, n_iter=int(n_iter), momentum=float(momentum))
