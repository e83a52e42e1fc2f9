"""The criteria of the reference's layers/hifigan_loss.py (:78-141) with its call signatures and return values.

Given the outputs of one call of MultiScaleDiscriminator / MultiPeriodDiscriminator (layers/hifigan.py: DiscOutputs) they read
that call's device reductions -- per sub-discriminator mean((1 - d_r)^2), mean(d_g^2), mean((1 - d_g)^2) and per layer
mean|f_r - f_g|, fixed partition and order, no float atomics -- and add the few scalars in the reference's order in fp32.
Lists of tensors of any other origin take the reference's arithmetic in torch.

mel_criterion is 45 x mean|mel(y_gt) - mel(y_pred)| with the extractor of :16-75 on the device (engine.MelLossEngine).  The
reference calls `y.squeeze()` first, which at B = 1 also drops the batch axis and breaks its own `y.unsqueeze(1)` padding call;
here [B,1,T] is always read as B waveforms.  The Slaney filterbank is librosa's (filters.mel defaults), restated; no librosa
exists on the build machine, so it is the one stage of the mel loss that is pinned by closed-form properties only."""
import torch
from torch import nn

from ..engine import MelLossEngine, l1_mean
from .hifigan import DiscOutputs


def _same_call(a, b, roles):
    return isinstance(a, DiscOutputs) and isinstance(b, DiscOutputs) and a.stats is b.stats and (a.role, b.role) == roles


class feature_criterion(nn.Module):
    def forward(self, fmap_r, fmap_g):
        if _same_call(fmap_r, fmap_g, ("f_r", "f_g")):
            st = fmap_r.stats.cpu()
            loss = torch.zeros((), dtype=torch.float32)
            for i in range(st.shape[0]):
                for l in range(3, st.shape[1]):
                    loss = loss + st[i, l]
            return (loss * 2).to(fmap_r.stats.device)
        loss = 0
        for dr, dg in zip(fmap_r, fmap_g):
            for rl, gl in zip(dr, dg):
                loss += torch.mean(torch.abs(rl - gl))
        return loss * 2


class discriminator_criterion(nn.Module):
    def forward(self, disc_real_outputs, disc_generated_outputs):
        if _same_call(disc_real_outputs, disc_generated_outputs, ("d_r", "d_g")):
            st = disc_real_outputs.stats.cpu()
            loss = torch.zeros((), dtype=torch.float32)
            for i in range(st.shape[0]):
                loss = loss + (st[i, 0] + st[i, 1])
            return loss.to(disc_real_outputs.stats.device), [float(v) for v in st[:, 0]], [float(v) for v in st[:, 1]]
        loss, r_losses, g_losses = 0, [], []
        for dr, dg in zip(disc_real_outputs, disc_generated_outputs):
            r_loss = torch.mean((1 - dr) ** 2)
            g_loss = torch.mean(dg ** 2)
            loss += r_loss + g_loss
            r_losses.append(r_loss.item())
            g_losses.append(g_loss.item())
        return loss, r_losses, g_losses


class generator_criterion(nn.Module):
    def forward(self, disc_outputs):
        if isinstance(disc_outputs, DiscOutputs) and disc_outputs.role == "d_g":
            st = disc_outputs.stats
            gen_losses = [st[i, 2] for i in range(st.shape[0])]
            c = st[:, 2].cpu()
            loss = torch.zeros((), dtype=torch.float32)
            for i in range(c.shape[0]):
                loss = loss + c[i]
            return loss.to(st.device), gen_losses
        loss, gen_losses = 0, []
        for dg in disc_outputs:
            l = torch.mean((1 - dg) ** 2)
            gen_losses.append(l)
            loss += l
        return loss, gen_losses


MEL_FIELDS = ("sample_rate", "fft_size", "num_mels", "mel_fmin", "mel_fmax", "win_length", "hop_length")


class mel_criterion(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        get = cfg.get if isinstance(cfg, dict) else (lambda k, d=None: getattr(cfg, k, d))
        defaults = dict(sample_rate=24000, fft_size=1024, num_mels=100, mel_fmin=0, mel_fmax=12000, win_length=1024, hop_length=256)
        self.args = {k: get(k, defaults[k]) for k in MEL_FIELDS}
        self._engine = None

    def extract_mel_features(self, y):
        """y [B,T] or [B,1,T] -> log-mel [B,num_mels,T // hop]"""
        if self._engine is None:
            self._engine = MelLossEngine(**self.args)
        return self._engine.forward(y.reshape(-1, y.shape[-1]).to(torch.float32).contiguous())

    @torch.inference_mode()
    def forward(self, y_gt, y_pred):
        return l1_mean(self.extract_mel_features(y_gt), self.extract_mel_features(y_pred), 45.0)
