"""CPU restatement of the HiFi-GAN generator with either residual block, for tests/test_hifigan_v1_host.py, tests/test_gpu_hifigan_v1.py
and scripts/make_hifigan_v1_golden.py (which pins it to the reference class, layers/hifigan.py:28-233).

    generator(sd, cfg, x)            x [B,d,T] -> [B,1,T * prod(upsample_rates)], in the dtype of x (fp32 or fp64)
    vocode_latents(sd, cfg, lat, s)  latents [B,n,d] -> F.interpolate(scale_factor=s, mode="linear") -> generator

`sd` is a state dict with the reference's names (conv_pre.weight_g / weight_v / bias, ups.{i}.*, resblocks.{i}.convs1.{m}.* and
.convs2.{m}.* for resblock_type "1", resblocks.{i}.convs.{q}.* otherwise, conv_post.*); weight norm is folded here
(w = g * v / |v|, the norm over every dimension but the first).  Nothing in this file touches the GPU."""
import torch
import torch.nn.functional as F

from genvc_amd import synth

SEED = 41
LRELU = 0.1
V1_KERNELS = [3, 7, 11]
V1_DILATIONS = [[1, 3, 5], [1, 3, 5], [1, 3, 5]]


def v1_cfg(upsample_initial_channel, upsample_rates, kernels=None, input_feat_dim=64):
    """a ResBlock1 generator config: transposed-conv kernels of twice the rate, the V1 dilations"""
    kernels = list(V1_KERNELS if kernels is None else kernels)
    return dict(input_feat_dim=input_feat_dim, upsample_initial_channel=upsample_initial_channel, resblock_kernel_sizes=kernels,
                resblock_dilation_sizes=[[1, 3, 5] for _ in kernels], upsample_rates=list(upsample_rates),
                upsample_kernel_sizes=[2 * r for r in upsample_rates], resblock_type="1")


# the fixture's generators: stage widths 128 and 64 / 32 (with input_feat_dim 64 every width of the one-round-trip conv kernel)
CFG_A = v1_cfg(256, [2, 2])
CFG_B = v1_cfg(64, [2])
# (tag, config, batch, input frames): 33 frames cross the 32- and 64-frame workgroup tiles after upsampling, the last tile ragged
CASES = [("a1", CFG_A, 1, 5), ("a2", CFG_A, 2, 33), ("b1", CFG_B, 1, 5), ("b2", CFG_B, 2, 33)]


def weights(cfg, seed=SEED, device="cpu"):
    return synth.make_weights(seed, synth.hifigan_weight_spec(cfg), device=device)


def frames(seed, B, T, d, name="mel"):
    """a generator input [B,d,T]"""
    return synth.uniform(seed, f"{name}_{B}_{T}_{d}", (B, d, T), 1.0)


def fold(sd, dtype=torch.float32):
    """weight-norm pairs -> plain weights, computed in `dtype`"""
    out = {}
    for k, v in sd.items():
        v = v.detach().cpu().to(dtype)
        if k.endswith(".weight_v"):
            g = sd[k[:-2] + "_g"].detach().cpu().to(dtype)
            norm = v.pow(2).sum(dim=tuple(range(1, v.dim())), keepdim=True).sqrt()
            out[k[:-9] + ".weight"] = g * v / norm
        elif not k.endswith(".weight_g"):
            out[k] = v
    return out


def _conv(w, name, x, k, dil):
    return F.conv1d(x, w[name + ".weight"], w[name + ".bias"], padding=dil * (k - 1) // 2, dilation=dil)


def resblock(w, name, x, k, dils, type1):
    if type1:                                      # per dilation: a dilated conv, then one of dilation 1, then the skip
        for m, d in enumerate(dils):
            t = _conv(w, f"{name}.convs1.{m}", F.leaky_relu(x, LRELU), k, d)
            x = _conv(w, f"{name}.convs2.{m}", F.leaky_relu(t, LRELU), k, 1) + x
        return x
    for q, d in enumerate(dils):
        x = _conv(w, f"{name}.convs.{q}", F.leaky_relu(x, LRELU), k, d) + x
    return x


def is_type1(cfg):
    return str(cfg.get("resblock_type", "2")) == "1"


@torch.inference_mode()
def generator(sd, cfg, x):
    w = fold(sd, x.dtype)
    kernels, dils = cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]
    nk = len(kernels)
    x = F.conv1d(x, w["conv_pre.weight"], w["conv_pre.bias"], padding=3)
    for i, (r, ku) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
        x = F.conv_transpose1d(F.leaky_relu(x, LRELU), w[f"ups.{i}.weight"], w[f"ups.{i}.bias"], stride=r, padding=(ku - r) // 2)
        xs = None
        for j, (k, ds) in enumerate(zip(kernels, dils)):
            y = resblock(w, f"resblocks.{i * nk + j}", x, k, ds, is_type1(cfg))
            xs = y if xs is None else xs + y
        x = xs / nk
    x = F.conv1d(F.leaky_relu(x), w["conv_post.weight"], w["conv_post.bias"], padding=3)        # (the default slope, 0.01)
    return torch.tanh(x)


@torch.inference_mode()
def vocode_latents(sd, cfg, latents, scale=4):
    mel = F.interpolate(latents.transpose(1, 2), scale_factor=[float(scale)], mode="linear")
    return generator(sd, cfg, mel)


def floor_of(a32, a64):
    """below this no fp32 result can be told from the fp64 one: the fp32 run's own error, or half an fp32 ulp of the largest entry"""
    a32, a64 = a32.detach().cpu().double(), a64.detach().cpu().double()
    return max(float((a32 - a64).abs().max()), 2.0 ** -24 * float(a64.abs().max()))


def reference(sd, cfg, x, fn=generator, **kw):
    """(fp32 result, floor from the fp64 run) of generator or vocode_latents"""
    y32 = fn(sd, cfg, x.float().cpu(), **kw)
    y64 = fn(sd, cfg, x.double().cpu(), **kw)
    return y32, floor_of(y32, y64)


def measured_receptive_frames(sd, cfg, T=None, d=None):
    """input frames on either side of an output sample that can reach it, measured: change one input frame in the middle of a long
    input and see which output samples move (a sample that the frame cannot reach is computed from identical values: it is bit-equal)"""
    up = 1
    for r in cfg["upsample_rates"]:
        up *= r
    d = cfg["input_feat_dim"] if d is None else d
    x = frames(SEED, 1, T, d, "rf")
    t = T // 2
    y0 = generator(sd, cfg, x)
    x1 = x.clone()
    x1[:, :, t] += 1.0
    moved = (generator(sd, cfg, x1) != y0).reshape(-1).nonzero().reshape(-1)
    lo, hi = int(moved.min()), int(moved.max())
    assert lo > 0 and hi < T * up - 1, "the input is too short to contain the receptive field"
    # output sample s belongs to input frame s / up: the farthest moved samples, in frames from the changed one
    return max(t - lo / up, (hi + 1) / up - (t + 1))
