"""CPU restatement, in torch, of the vocoder trainer's evaluation step (reference trainers/hifigan_trainer.py:346-385): the two
waveform-domain discriminators of layers/hifigan.py (:247-426) in eval mode with both weight folds, the four criteria of
layers/hifigan_loss.py (:78-141) and that file's mel extractor (:16-75) with librosa's default (Slaney) filterbank restated.

scripts/make_vocoder_eval_golden.py asserts that this file matches the reference's own classes within the fp32-vs-fp64 floor of
each quantity; the filterbank is the one stage nothing on the build machine can pin (no librosa), so the host tests check its
closed-form properties instead.  Everything is dtype-generic: weights and inputs in float64 give the float64 result."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from genvc_amd import synth

LRELU_SLOPE = 0.1
MSD_CONVS = [(128, 1, 15, 1, 1, 7), (128, 128, 41, 2, 4, 20), (256, 128, 41, 2, 16, 20), (512, 256, 41, 4, 16, 20),
             (1024, 512, 41, 4, 16, 20), (1024, 1024, 41, 1, 16, 20), (1024, 1024, 5, 1, 1, 2)]      # (out, in, k, stride, groups, pad)
MEL_CFG = dict(sample_rate=24000, fft_size=1024, num_mels=100, mel_fmin=0, mel_fmax=12000, win_length=1024, hop_length=256)
SEED = 31


# ---- inputs and weights shared by the fixture script and the tests ---------------------------------------------------------------
def wav_pair(seed, B, T, device="cpu"):
    """real and generated waveform [B,1,T]: two different synth_audio draws per item (amplitudes 0.3 / 0.25)"""
    y = torch.stack([synth.synth_audio(seed, f"real{b}", T, 0.3) for b in range(B)]).view(B, 1, T)
    g = torch.stack([synth.synth_audio(seed, f"gen{b}", T, 0.25) for b in range(B)]).view(B, 1, T)
    return y.to(device), g.to(device)


def mpd_cfg(mult=1, periods=(2, 3, 5, 7, 11), spectral=False):
    return dict(mpd_reshapes=list(periods), mpd_discriminator_channel_mult_factor=mult, mpd_use_spectral_norm=spectral)


def msd_weights(seed=SEED, device="cpu"):
    return synth.make_weights(seed, synth.msd_weight_spec(), device=device)


def mpd_weights(cfg, seed=SEED, device="cpu"):
    return synth.make_weights(seed, synth.mpd_weight_spec(cfg), device=device)


def cpu_state(module):
    return {k: v.detach().cpu() for k, v in module.state_dict().items()}


def subsample(fm):
    """what the fixture keeps of a feature map [B,C,...]: every ceil(C / 16)-th channel and every ceil(frames / 16)-th frame of the
    flattened trailing axes (the first layers are megabytes otherwise)"""
    fm = fm.reshape(fm.shape[0], fm.shape[1], -1)
    return fm[:, ::-(-fm.shape[1] // 16), ::-(-fm.shape[2] // 16)]


# the fixture's cases: (tag, B, T, MPD channel multiplier).  4096 is divisible by 2 only (reflect pads of 2, 4, 6, 7 samples for the
# periods 3, 5, 7, 11), 3072 by 2 and 3
CASES = [("a", 2, 4096, 1), ("b", 1, 3072, 0.25)]


# ---- weight folds ------------------------------------------------------------------------------------------------------------------
def fold_weight_norm(g, v):
    """torch.nn.utils.weight_norm (dim 0): w = v * (g / |v|), the norm over everything but the output channel"""
    return torch._weight_norm(v, g, 0)


def fold_spectral_norm(orig, u, v):
    """torch.nn.utils.spectral_norm in eval mode: weight_orig / sigma, sigma = u . (W_mat v) with the stored u, v"""
    sigma = torch.dot(u, torch.mv(orig.reshape(orig.shape[0], -1), v))
    return orig / sigma


def folded(sd, name):
    if name + ".weight_orig" in sd:
        return fold_spectral_norm(sd[name + ".weight_orig"], sd[name + ".weight_u"], sd[name + ".weight_v"])
    return fold_weight_norm(sd[name + ".weight_g"], sd[name + ".weight_v"])


# ---- discriminators ----------------------------------------------------------------------------------------------------------------
def disc_s(sd, i, x):
    fmap = []
    p = f"discriminators.{i}."
    for j, (_, _, _, stride, groups, pad) in enumerate(MSD_CONVS):
        x = F.leaky_relu(F.conv1d(x, folded(sd, f"{p}convs.{j}"), sd[f"{p}convs.{j}.bias"], stride=stride, padding=pad, groups=groups),
                         LRELU_SLOPE)
        fmap.append(x)
    x = F.conv1d(x, folded(sd, p + "conv_post"), sd[p + "conv_post.bias"], padding=1)
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def msd(sd, y, y_hat):
    d_r, d_g, f_r, f_g = [], [], [], []
    for i in range(3):
        if i:
            y, y_hat = F.avg_pool1d(y, 4, 2, padding=2), F.avg_pool1d(y_hat, 4, 2, padding=2)
        r, fr = disc_s(sd, i, y)
        g, fg = disc_s(sd, i, y_hat)
        d_r.append(r); d_g.append(g); f_r.append(fr); f_g.append(fg)
    return d_r, d_g, f_r, f_g


def disc_p(sd, i, period, x):
    fmap = []
    p = f"discriminators.{i}."
    b, c, t = x.shape
    if t % period:
        n_pad = period - t % period
        x = F.pad(x, (0, n_pad), "reflect")
        t += n_pad
    x = x.view(b, c, t // period, period)
    for j in range(5):
        # (all five convs have stride (3, 1) and padding get_padding(5, 1) = 2 in the reference, :324-369 -- the original HiFi-GAN's
        # fifth conv has stride 1)
        x = F.leaky_relu(F.conv2d(x, folded(sd, f"{p}convs.{j}"), sd[f"{p}convs.{j}.bias"], stride=(3, 1), padding=(2, 0)),
                         LRELU_SLOPE)
        fmap.append(x)
    x = F.conv2d(x, folded(sd, p + "conv_post"), sd[p + "conv_post.bias"], padding=(1, 0))
    fmap.append(x)
    return torch.flatten(x, 1, -1), fmap


def mpd(sd, periods, y, y_hat):
    d_r, d_g, f_r, f_g = [], [], [], []
    for i, period in enumerate(periods):
        r, fr = disc_p(sd, i, period, y)
        g, fg = disc_p(sd, i, period, y_hat)
        d_r.append(r); d_g.append(g); f_r.append(fr); f_g.append(fg)
    return d_r, d_g, f_r, f_g


# ---- criteria ----------------------------------------------------------------------------------------------------------------------
def feature_means(fmap_r, fmap_g):
    return [[torch.mean(torch.abs(rl - gl)) for rl, gl in zip(dr, dg)] for dr, dg in zip(fmap_r, fmap_g)]


def feature_criterion(fmap_r, fmap_g):
    loss = 0
    for row in feature_means(fmap_r, fmap_g):
        for v in row:
            loss = loss + v
    return loss * 2


def discriminator_criterion(d_r, d_g):
    loss, r_losses, g_losses = 0, [], []
    for dr, dg in zip(d_r, d_g):
        r_loss, g_loss = torch.mean((1 - dr) ** 2), torch.mean(dg ** 2)
        loss = loss + (r_loss + g_loss)
        r_losses.append(float(r_loss)); g_losses.append(float(g_loss))
    return loss, r_losses, g_losses


def generator_criterion(d_g):
    loss, gen = 0, []
    for dg in d_g:
        l = torch.mean((1 - dg) ** 2)
        gen.append(l)
        loss = loss + l
    return loss, gen


# ---- mel loss ----------------------------------------------------------------------------------------------------------------------
F_SP = 200.0 / 3.0
MIN_LOG_HZ = 1000.0
MIN_LOG_MEL = MIN_LOG_HZ / F_SP
LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(f):
    """Slaney's scale (librosa.hz_to_mel, htk=False): linear below 1 kHz, logarithmic above"""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= MIN_LOG_HZ, MIN_LOG_MEL + np.log(np.maximum(f, 1e-30) / MIN_LOG_HZ) / LOGSTEP, f / F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= MIN_LOG_MEL, MIN_LOG_HZ * np.exp(LOGSTEP * (m - MIN_LOG_MEL)), F_SP * m)


def mel_centres(n_mels, fmin, fmax):
    """the n_mels + 2 band edges / centres in Hz, equally spaced on the mel scale"""
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))


def slaney_filterbank(sr, n_fft, n_mels, fmin, fmax):
    """librosa.filters.mel(sr=, n_fft=, n_mels=, fmin=, fmax=) with its defaults (htk=False, norm='slaney') -> float32
    [n_mels, 1 + n_fft // 2]: triangles between neighbouring centres, each scaled by 2 / (its band width in Hz)"""
    fft_f = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_centres(n_mels, fmin, fmax)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.zeros((n_mels, fft_f.size))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
    w *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return w.astype(np.float32)


def extract_mel_features(y, cfg=MEL_CFG, basis=None):
    """y [B,T] -> [B,num_mels,T // hop]: reflect padding of (fft_size - hop) / 2, center=False, sqrt(re^2 + im^2 + 1e-9), the
    filterbank, log(clamp(., 1e-5))"""
    if basis is None:
        basis = torch.from_numpy(slaney_filterbank(cfg["sample_rate"], cfg["fft_size"], cfg["num_mels"], cfg["mel_fmin"], cfg["mel_fmax"]))
    basis = basis.to(y.dtype)
    pad = int((cfg["fft_size"] - cfg["hop_length"]) / 2)
    y = F.pad(y.unsqueeze(1), (pad, pad), mode="reflect").squeeze(1)
    spec = torch.stft(y, cfg["fft_size"], hop_length=cfg["hop_length"], win_length=cfg["win_length"],
                      window=torch.hann_window(cfg["win_length"], dtype=y.dtype, device=y.device), center=False, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)
    spec = torch.sqrt(torch.view_as_real(spec).pow(2).sum(-1) + 1e-9)
    return torch.log(torch.clamp(torch.matmul(basis, spec), min=1e-5))


def mel_criterion(y_gt, y_pred, cfg=MEL_CFG):
    """[B,1,T] or [B,T]: always B waveforms (the reference's y.squeeze() also drops the batch axis at B = 1 and then fails)"""
    a = extract_mel_features(y_gt.reshape(-1, y_gt.shape[-1]), cfg)
    b = extract_mel_features(y_pred.reshape(-1, y_pred.shape[-1]), cfg)
    return F.l1_loss(a, b) * 45
