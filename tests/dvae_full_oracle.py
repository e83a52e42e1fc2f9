"""CPU restatement of the acoustic DiscreteVAE's eval-mode methods (reference layers/dvae.py:333-381) in plain torch, with the
nearest-x2 upsampling + Conv1d stages written as the polyphase convs the library runs: output frame 2m + ph =
sum_o (sum_{j : floor((ph - p + j) / 2) = o} W_j) x[m + o], p = (k - 1) / 2, x zero outside [0, n).  The encoder and the VQ are the
oracle's (oracle/genvc_oracle.py); tests/golden/acoustic_dvae_*.npz pin all of it to the reference's own class."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import genvc_oracle as O      # noqa: E402

# train_genVC.py:14-25 and a small variant of the same depth
FULL = dict(num_channels=80, num_tokens=1024, codebook_dim=512, hidden_dim=512, num_resnet_blocks=3, kernel_size=3, num_layers=2)
TINY = dict(FULL, codebook_dim=64, hidden_dim=32, num_resnet_blocks=1)
K5 = dict(FULL, codebook_dim=64, hidden_dim=64, num_resnet_blocks=1, kernel_size=5, num_layers=3)
CODEBOOK_SCALE = 0.05
MEL_1024 = dict(n_fft=1024, hop=256, win=1024, sr=24000, f_min=0.0, f_max=8000.0, n_mels=80)


def fold_upconv(w):
    """w [Co,Ci,k] -> [(first tap offset, folded weight [Co,Ci,p+1])] for the even and the odd output frames"""
    k = w.shape[-1]
    p = (k - 1) // 2
    out = []
    for ph in (0, 1):
        omin = (ph - p) // 2                    # (Python's // floors)
        wf = torch.zeros(w.shape[0], w.shape[1], p + 1, dtype=w.dtype)
        for j in range(k):
            wf[:, :, (ph - p + j) // 2 - omin] += w[:, :, j]
        out.append((omin, wf))
    return out


def upconv_polyphase(x, w, b):
    """relu(conv1d(interpolate(x, 2, nearest), w, b, padding=(k-1)/2)) without the upsampled tensor: x [B,Ci,n] -> [B,Co,2n]"""
    B, _, n = x.shape
    y = torch.empty(B, w.shape[0], 2 * n, dtype=x.dtype)
    for ph, (omin, wf) in enumerate(fold_upconv(w)):
        nt = wf.shape[-1]
        xp = F.pad(x, (-omin, omin + nt - 1))                         # frame m + omin + t of x at index m + t
        y[:, :, ph::2] = F.conv1d(xp, wf, b)
    return F.relu(y)


def decode(w, cfg, codes, prefix=""):
    """codes int64 [B,n] -> (out [B,channels,n 2^L], the last layer's input [B,hidden,n 2^L])"""
    x = F.embedding(codes, w[prefix + "codebook.embed"].t()).permute(0, 2, 1)
    idx = 0
    g = lambda name: (w[f"{prefix}decoder.{name}.weight"], w[f"{prefix}decoder.{name}.bias"])
    if cfg["num_resnet_blocks"] > 0:
        x = F.conv1d(x, *g("0"))
        idx = 1
    for _ in range(cfg["num_resnet_blocks"]):
        h = F.relu(F.conv1d(x, *g(f"{idx}.net.0"), padding=1))
        h = F.relu(F.conv1d(h, *g(f"{idx}.net.2"), padding=1))
        x = F.conv1d(h, *g(f"{idx}.net.4")) + x
        idx += 1
    for _ in range(cfg["num_layers"]):
        x = upconv_polyphase(x, *g(f"{idx}.0.conv"))
        idx += 1
    return F.conv1d(x, *g(str(idx))), x


def forward(w, cfg, feat, prefix=""):
    """eval-mode forward: feat [B,C,T] -> (recon_loss, commitment_loss, out, codes)"""
    enc = O.dvae_encode(w, feat, prefix)
    codes = O.vq_indices(enc, w[prefix + "codebook.embed"])
    q = F.embedding(codes, w[prefix + "codebook.embed"].t())
    out, _ = decode(w, cfg, codes, prefix)
    return F.mse_loss(feat, out), (q - enc).pow(2).mean(), out, codes


def mel_1024(wav, mel_norms):
    """the DVAE's extractor (TorchMelSpectrogram defaults, utils.py:97-162: n_fft 1024, hop 256, win 1024): wav [B,T] -> [B,80,1+T//256]"""
    c = MEL_1024
    window = torch.hann_window(c["win"], periodic=True)
    spec = torch.stft(wav.float(), c["n_fft"], c["hop"], c["win"], window=window, center=True, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)
    power = spec.real ** 2 + spec.imag ** 2
    fb = O.mel_filterbank(c["n_fft"] // 2 + 1, c["f_min"], c["f_max"], c["n_mels"], c["sr"])
    mel = torch.matmul(power.transpose(1, 2), fb).transpose(1, 2)
    return torch.log(torch.clamp(mel, min=1e-5)) / mel_norms.float().view(1, -1, 1)


def designed_codes(seed, B, n, num_tokens):
    """decoder inputs: hashed codes with the first and the last code and runs of repeated neighbours placed in"""
    from genvc_amd import synth
    c = synth.integers(seed, f"dec_codes_{B}_{n}", (B, n), num_tokens)
    c[0, 0] = 0
    c[-1, -1] = num_tokens - 1
    if n >= 4:
        c[:, 2] = c[:, 1]
        c[0, n // 2] = num_tokens - 1
        c[-1, n // 2 - 1] = 0
    if n >= 8:
        c[:, n - 4:n - 1] = c[:, n - 4:n - 3]
    return c


WAV_AMPLITUDES = (0.1, 0.4)            # a quiet and a loud item: more distinct codes per batch than two equal ones


def acoustic_wavs(seed, tag, n, B=2):
    """the fixtures' waveforms [B,n]: synth_audio per item at WAV_AMPLITUDES"""
    from genvc_amd import synth
    return torch.cat([synth.synth_audio(seed, f"acoustic_{tag}_{n}_{i}", n, amplitude=WAV_AMPLITUDES[i % 2]) for i in range(B)])
