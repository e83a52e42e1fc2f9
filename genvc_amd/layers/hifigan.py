"""HiFi-GAN generator with the reference's constructor and `forward(x[B,d,T]) -> [B,1,256T]`
(/root/reference/layers/hifigan.py:160-233) on libgenvc_hip (gvc_hifigan_forward).  Holds the
weight-norm parametrised tensors under the reference's names (conv_pre.weight_g/_v, ups.{i}.*, resblocks.*), with either residual
block: ResBlock2 (resblocks.{i}.convs.{0,1}) or, for resblock_type "1", ResBlock1 (resblocks.{i}.convs1.{m} / convs2.{m}, :28-117).

MultiScaleDiscriminator and MultiPeriodDiscriminator (:247-426) in eval mode on gvc_disc_forward; the STFT and CQT
discriminators (:429-) are not served."""
import torch
from torch import nn

from ..engine import DiscriminatorEngine, HifiganEngine, mpd_channels


class _Holder(nn.Module):
    pass


def _wn(shape, bias_n):
    m = _Holder()
    m.weight_g = nn.Parameter(torch.ones(shape[0], 1, 1), requires_grad=False)
    m.weight_v = nn.Parameter(torch.empty(*shape).normal_(std=0.01), requires_grad=False)
    m.bias = nn.Parameter(torch.zeros(bias_n), requires_grad=False)
    return m


class HiFiGAN(nn.Module):
    def __init__(self, input_feat_dim, upsample_initial_channel, resblock_kernel_sizes, resblock_dilation_sizes,
                 upsample_rates, upsample_kernel_sizes, resblock_type="1"):
        super().__init__()
        # the reference's rule (:181): "1" is ResBlock1 (convs1 / convs2, three dilations per kernel), anything else ResBlock2
        type1 = str(resblock_type) == "1"
        for d in resblock_dilation_sizes:
            if len(d) != (3 if type1 else 2):
                raise ValueError(f"HiFiGAN: ResBlock{1 if type1 else 2} takes {3 if type1 else 2} dilations per kernel, got {list(d)}")
        self.cfg = dict(input_feat_dim=input_feat_dim, upsample_initial_channel=upsample_initial_channel,
                        resblock_kernel_sizes=list(resblock_kernel_sizes),
                        resblock_dilation_sizes=[list(d) for d in resblock_dilation_sizes],
                        upsample_rates=list(upsample_rates), upsample_kernel_sizes=list(upsample_kernel_sizes),
                        resblock_type="1" if type1 else "2")
        ch = upsample_initial_channel
        self.conv_pre = _wn((ch, input_feat_dim, 7), ch)
        self.ups = nn.ModuleList()
        self.resblocks = nn.ModuleList()
        for r, k in zip(upsample_rates, upsample_kernel_sizes):
            self.ups.append(_wn((ch, ch // 2, k), ch // 2))
            ch //= 2
            for kk in resblock_kernel_sizes:
                rb = _Holder()
                if type1:
                    rb.convs1 = nn.ModuleList([_wn((ch, ch, kk), ch) for _ in range(3)])
                    rb.convs2 = nn.ModuleList([_wn((ch, ch, kk), ch) for _ in range(3)])
                else:
                    rb.convs = nn.ModuleList([_wn((ch, ch, kk), ch), _wn((ch, ch, kk), ch)])
                self.resblocks.append(rb)
        self.conv_post = _wn((1, ch, 7), 1)
        self._engine = None

    def bind(self, max_batch=2, max_frames=2560):
        if self._engine is not None:
            self._engine.close()
        self._engine = HifiganEngine(self.cfg, max_batch=max_batch, max_frames=max_frames)
        self._engine.bind(dict(self.state_dict()))
        return self

    # frames of context kept on each side of a window of a long input: the generator's receptive field is +-13 input frames
    # (conv_pre 3, the k = 7 / dilation 12 ResBlock of the first upsampling stage 6, the rest < 1 each)
    def receptive_frames(self):
        """input frames on either side that can reach one output sample (reference hifigan.py:119-157,218-233: conv_pre k = 7, per
        stage a transposed conv of kernel k_up at the stage's output rate and ResBlock2s whose two dilated convs reach
        (k - 1) / 2 * d samples each; conv_post k = 7): 10.66 frames for the trained configuration.  A ResBlock1 (:28-117) follows each
        dilated conv with one of dilation 1: (k - 1) / 2 * d + (k - 1) / 2 per dilation"""
        rf, cum = 3.0, 1.0
        own = 1 if self.cfg["resblock_type"] == "1" else 0          # the dilation-1 conv behind every dilated one
        for r, ku in zip(self.cfg["upsample_rates"], self.cfg["upsample_kernel_sizes"]):
            cum *= r
            reach = max(sum((k - 1) // 2 * (d + own) for d in ds) for k, ds in zip(self.cfg["resblock_kernel_sizes"], self.cfg["resblock_dilation_sizes"]))
            rf += (ku / 2.0 + reach) / cum
        return rf + 3.0 / cum

    @property
    def window_overlap(self):
        """frames re-computed on either side of a window's kept interior: the receptive field rounded up to a multiple of 8 plus
        a margin (32 for the trained configuration)"""
        import math
        return int(math.ceil((self.receptive_frames() + 8) / 8.0)) * 8 + 8

    @torch.inference_mode()
    def forward(self, x):
        """x [B,d,T] -> [B,1,T * prod(upsample_rates)].  The reference has no length limit (non-streaming conversion vocodes the
        latents of ALL segments in one call, inference_utils.py:79-87): inputs beyond the engine's buffers go through it in
        overlapping windows whose interiors are stitched (every kept sample sees its full receptive field)."""
        if self._engine is None:
            self.bind()
        x = x.to(torch.float32)
        T, cap, ov = x.shape[-1], self._engine.max_frames, self.window_overlap
        if T <= cap:
            return self._engine.forward(x.contiguous())
        if cap <= 2 * ov + 8:
            raise ValueError(f"HiFiGAN: {T} frames exceed the engine's buffers ({cap} frames) and those are too small for overlapping "
                             f"windows (receptive field {self.receptive_frames():.1f} frames, overlap {ov}): bind(max_frames=...) larger")
        up = 1
        for r in self.cfg["upsample_rates"]:
            up *= r
        core = cap - 2 * ov
        out = []
        for s in range(0, T, core):
            lo, hi = max(0, s - ov), min(T, s + core + ov)
            y = self._engine.forward(x[:, :, lo:hi].contiguous())
            n = min(core, T - s)
            out.append(y[:, :, (s - lo) * up:(s - lo + n) * up].clone())
        return torch.cat(out, dim=-1)

    @torch.inference_mode()
    def forward_latents(self, latents, scale=4):
        """latents [B,n,d] -> wav; fuses the harness's F.interpolate(scale_factor=4, mode='linear')"""
        if self._engine is None:
            self.bind()
        latents = latents.to(torch.float32)
        if latents.shape[1] * scale > self._engine.max_frames:      # long input: the reference's own interpolation call, then windows
            mel = torch.nn.functional.interpolate(latents.transpose(1, 2), scale_factor=[float(scale)], mode="linear")
            return self.forward(mel)
        return self._engine.forward_latents(latents.contiguous(), scale)


# ---- discriminators (eval mode) ------------------------------------------------------------------------------------------------
def _disc_conv(shape, spectral):
    """parameters of one discriminator conv as torch's weight_norm / spectral_norm leave them in a state dict (same names, kinds
    and order: bias, then weight_g + weight_v, or weight_orig with the buffers weight_u + weight_v)"""
    m = _Holder()
    co = shape[0]
    m.bias = nn.Parameter(torch.zeros(co), requires_grad=False)
    if spectral:
        m.weight_orig = nn.Parameter(torch.empty(*shape).normal_(std=0.01), requires_grad=False)
        r = m.weight_orig[0].numel()
        m.register_buffer("weight_u", torch.nn.functional.normalize(torch.randn(co), dim=0))
        m.register_buffer("weight_v", torch.nn.functional.normalize(torch.randn(r), dim=0))
    else:
        m.weight_g = nn.Parameter(torch.ones(co, *([1] * (len(shape) - 1))), requires_grad=False)
        m.weight_v = nn.Parameter(torch.empty(*shape).normal_(std=0.01), requires_grad=False)
    return m


class DiscOutputs(list):
    """a list of logits or of feature-map lists that remembers the call it came from: `stats` [n_sub, 3 + n_layers] are that
    call's device reductions (DiscriminatorEngine.forward), `role` is "d_r", "d_g", "f_r" or "f_g".  The criteria of
    layers/hifigan_loss.py read the reductions instead of the tensors when both arguments come from one call."""

    def __init__(self, items, stats, role):
        super().__init__(items)
        self.stats, self.role = stats, role


class _Discriminator(nn.Module):
    kind = ""

    def _engine_args(self):
        raise NotImplementedError

    def bind(self, max_batch=2, max_samples=24000):
        if self._engine is not None:
            self._engine.close()
        self._engine = DiscriminatorEngine(self.kind, max_batch=max_batch, max_samples=max_samples, **self._engine_args())
        self._engine.bind(dict(self.state_dict()))
        return self

    @torch.inference_mode()
    def forward(self, y, y_hat):
        """y, y_hat [B,1,T] -> (y_d_rs, y_d_gs, fmap_rs, fmap_gs) with the reference's shapes.  The tensors are views of the
        engine's buffers: the next forward of this module overwrites them."""
        if self.training:
            raise NotImplementedError(f"{type(self).__name__} runs in eval mode only (call .eval()): training-mode spectral norm "
                                      "updates weight_u per call and there are no gradients")
        B, T = y.shape[0], y.shape[-1]
        if self._engine is None or B > self._engine.max_batch or T > self._engine.max_samples:
            self.bind(max_batch=max(B, 2), max_samples=max(T, 24000))
        eng = self._engine
        stats = eng.forward(y.reshape(B, T).to(torch.float32).contiguous(), y_hat.reshape(B, T).to(torch.float32).contiguous())
        d_r, d_g, f_r, f_g = [], [], [], []
        for i in range(eng.n_sub):
            maps = [eng.layer(i, l, B, T) for l in range(eng.n_layers)]
            if self.kind == "MSD":
                maps = [m.squeeze(-1) for m in maps]
            f_r.append([m[:B] for m in maps])
            f_g.append([m[B:] for m in maps])
            d_r.append(maps[-1][:B].flatten(1, -1))
            d_g.append(maps[-1][B:].flatten(1, -1))
        return (DiscOutputs(d_r, stats, "d_r"), DiscOutputs(d_g, stats, "d_g"), DiscOutputs(f_r, stats, "f_r"),
                DiscOutputs(f_g, stats, "f_g"))


class MultiScaleDiscriminator(_Discriminator):
    """reference layers/hifigan.py:281-314: 3 x DiscriminatorS (the first under spectral norm), AvgPool1d(4, 2, padding=2) between"""
    kind = "MSD"
    CONVS = [(128, 1, 15), (128, 32, 41), (256, 8, 41), (512, 16, 41), (1024, 32, 41), (1024, 64, 41), (1024, 1024, 5)]

    def __init__(self):
        super().__init__()
        self.discriminators = nn.ModuleList()
        for i in range(3):
            d = _Holder()
            d.convs = nn.ModuleList([_disc_conv(s, i == 0) for s in self.CONVS])
            d.conv_post = _disc_conv((1, 1024, 3), i == 0)
            self.discriminators.append(d)
        self._engine = None

    def _engine_args(self):
        return {}


class MultiPeriodDiscriminator(_Discriminator):
    """reference layers/hifigan.py:399-426: one DiscriminatorP per period of mpd_reshapes"""
    kind = "MPD"

    def __init__(self, mpd_reshapes, mpd_discriminator_channel_mult_factor, mpd_use_spectral_norm):
        super().__init__()
        self.mpd_reshapes = list(mpd_reshapes)
        self.d_mult, self.use_spectral_norm = mpd_discriminator_channel_mult_factor, bool(mpd_use_spectral_norm)
        self.discriminators = nn.ModuleList()
        for _ in self.mpd_reshapes:
            d = _Holder()
            d.convs = nn.ModuleList()
            cin = 1
            for co in mpd_channels(self.d_mult):
                d.convs.append(_disc_conv((co, cin, 5, 1), self.use_spectral_norm))
                cin = co
            d.conv_post = _disc_conv((1, cin, 3, 1), self.use_spectral_norm)
            self.discriminators.append(d)
        self._engine = None

    def _engine_args(self):
        return dict(periods=self.mpd_reshapes, mult=self.d_mult, spectral_norm=self.use_spectral_norm)


def _unserved(name):
    class _Unserved(nn.Module):
        def __init__(self, *a, **k):
            raise NotImplementedError(f"{name} is not served: it needs a spectrogram / CQT front end and 2-D convolutions "
                                      "(MultiScaleDiscriminator and MultiPeriodDiscriminator are)")
    _Unserved.__name__ = _Unserved.__qualname__ = name
    return _Unserved


MultiScaleSTFTDiscriminator = _unserved("MultiScaleSTFTDiscriminator")
MultiScaleSubbandCQTDiscriminator = _unserved("MultiScaleSubbandCQTDiscriminator")
