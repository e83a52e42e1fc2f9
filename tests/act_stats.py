"""Trained-model activation ranges for the GPT and encoder parity tests (test infrastructure only).

`synth.make_weights` gives activations far tamer than a trained checkpoint's: residual rows centred at zero, no outlier channel,
LayerNorm gains near 1 and attention scores with a std of about 0.4 (every softmax close to uniform).  The kernels that fold
LayerNorm into a projection, merge online-softmax chunks or round to bf16 are only sensitive where those weights never go.  This
module turns synthetic weights and inputs into trained-like ones with independent knobs:

  offset    a fixed vector of mean `offset` and spread ~1 on every embedding row and conditioning latent: every residual row carries
            it into each LN1, LN2, ln_f and final_norm (|mean| / std of the LayerNorm inputs ~ offset)
  outliers  a few channels of magnitude 50..500 in the embeddings, grown with depth through each layer's mlp.c_proj.bias (GPT-2's
            "massive activations"), with small LayerNorm gains on those channels
  ln        LayerNorm gains spread over [0.05, 3], biases of std 0.3
  peaked    q and k projections scaled so the attention scores have a std of about `peaked`: peaked softmaxes, rows whose
            score range passes 88 (exp(s) overflows without max subtraction, whole key chunks underflow to 0)
  dc        (waveforms) a DC offset and a stretch of constant non-zero samples on the ContentVec input

`record()` collects, from an oracle run (float64 in the tests), the statistics each knob must reach; `yardstick()` is the
tolerance rule of the GPU tests: a kernel's deviation from the float64 oracle against the float32 oracle's own deviation and
against the kernel's deviation on the default weights."""
import contextlib
import math

import torch
import torch.nn.functional as F

from genvc_amd import synth

OUTLIER_MAG = (40.0, -90.0, 200.0)          # in the embeddings; the c_proj biases double them over the depth (up to 400)

PRESETS = {
    "default": {},
    "offset": dict(offset=300.0),
    "offset30": dict(offset=30.0),
    "outliers": dict(outliers=OUTLIER_MAG),
    "ln": dict(ln=True),
    "peaked": dict(peaked=20.0),
    "all": dict(offset=300.0, outliers=OUTLIER_MAG, ln=True, peaked=36.0),   # (outlier channels take most of a row's variance)
}

# what a preset must reach under the float64 oracle (checked by `check_regime`)
#   ln_ratio: median over LayerNorm calls of the median row |mean| / std;  max_abs: largest |x| at a LayerNorm input;
#   spread: largest max - min of the finite scores of one softmax row;  score_std: median over softmax calls of the score std;
#   gn_ratio: largest |mean| / std of a GroupNorm group (ContentVec's first conv layer: one channel over time)
REGIMES = {
    "offset": dict(ln_ratio=100.0),
    "offset30": dict(ln_ratio=10.0),
    "outliers": dict(max_abs=150.0),
    "peaked": dict(spread=88.0, score_std=5.0),
    "all": dict(ln_ratio=20.0, max_abs=150.0, spread=88.0, score_std=5.0),
    "dc": dict(gn_ratio=100.0),
}


def knobs(preset):
    return dict(PRESETS[preset]) if isinstance(preset, str) else dict(preset)


def _u(seed, name, shape, std, mean=0.0):
    return synth.uniform(seed, "act_stats." + name, shape, std, mean).double()


def outlier_channels(d):
    """three fixed, well-separated channels"""
    return [d // 7, (3 * d) // 5, d - 11]


def row_shift(d, preset, seed=0):
    """the vector every embedding row and conditioning latent carries (float64, [d]) or None"""
    k = knobs(preset)
    v = None
    if k.get("offset"):
        v = _u(seed, "offset", (d,), 1.0, float(k["offset"]))
    if k.get("outliers"):
        v = torch.zeros(d, dtype=torch.float64) if v is None else v
        for c, m in zip(outlier_channels(d), k["outliers"]):
            v[c] += m
    return v


def _put(out, name, t64):
    out[name] = t64.to(dtype=out[name].dtype, device=out[name].device)


def _ln_gain_bias(out, name, d, seed, k, chans):
    if k.get("ln"):
        g = 0.05 + 2.95 * (_u(seed, name + ".g", (d,), 1.0 / math.sqrt(12.0), 0.5))
        _put(out, name + ".weight", g)
        _put(out, name + ".bias", _u(seed, name + ".b", (d,), 0.3))
    if chans:
        g = out[name + ".weight"].double().cpu().clone()
        g[chans] = 0.05
        _put(out, name + ".weight", g)


def gpt_weights(w, dims, preset, seed=0):
    """a trained-like copy of GPT weights `w` (any device / float dtype; the dtype and device are kept)"""
    k = knobs(preset)
    out = dict(w)
    d, L, H = dims["d_model"], dims["n_layer"], dims["n_head"]
    chans = outlier_channels(d) if k.get("outliers") else []
    v = row_shift(d, k, seed)
    if v is not None:          # half on the token table, half on the position table: every row carries v once
        for t in ("text_embedding.weight", "text_pos_embedding.emb.weight", "mel_embedding.weight", "mel_pos_embedding.emb.weight"):
            _put(out, t, out[t].double().cpu() + 0.5 * v)
    lns = [f"gpt.h.{l}.ln_{i}" for l in range(L) for i in (1, 2)] + ["gpt.ln_f", "final_norm"]
    for n in lns:
        _ln_gain_bias(out, n, d, seed, k, chans)
    if chans:
        for l in range(L):
            b = out[f"gpt.h.{l}.mlp.c_proj.bias"].double().cpu().clone()
            for c, m in zip(chans, k["outliers"]):
                b[c] += m / L
            _put(out, f"gpt.h.{l}.mlp.c_proj.bias", b)
    if k.get("peaked"):
        # each layer's q and k column blocks scaled by alpha_l, calibrated on a float64 prefill of a fixed input (LayerNorm outputs are not
        # unit-variance per channel once outlier channels take most of a row's variance, so no closed form fits every preset)
        cond = cond_latents(synth.uniform(0, "act_stats.calib_cond", (1, 32, d), 1.0), d, k, seed)
        codes = synth.integers(0, "act_stats.calib_codes", (1, 13), 256)

        def run(ww):
            from oracle import genvc_oracle as O
            O.gpt_prefill(ww, dims, O.compute_embeddings(ww, dims, cond.double(), codes)[0])

        def scale(ww, l, alpha):
            p = f"gpt.h.{l}.attn.c_attn."
            for n in ("weight", "bias"):
                t = ww[p + n].double().cpu().clone()
                t[..., :2 * d] *= alpha
                _put(ww, p + n, t)
        out = _calibrate(out, run, L, scale, float(k["peaked"]))
    return out


def cond_latents(cond, d, preset, seed=0):
    """conditioning latents [B,32,d] carrying the preset's row shift"""
    v = row_shift(d, preset, seed)
    if v is None:
        return cond
    return (cond.double() + v.to(cond.device)).to(cond.dtype)


def double(w):
    return {n: t.detach().cpu().double() for n, t in w.items()}


def single(w):
    return {n: t.detach().cpu().float() for n, t in w.items()}


# ---------------------------------------------------------------------------
# encoders: calibrated q / k scaling, DC on the waveform
# ---------------------------------------------------------------------------

def _calibrate(w, run, n_layers, scale, target, passes=3):
    """scale(w, l, alpha) multiplies layer l's q and k projections by alpha; run(float64 weights) runs the oracle once, one softmax
    call per layer in layer order.  Each pass brings every layer's score std to about `target`."""
    out = dict(w)
    for _ in range(passes):
        with record() as st:
            run(double(out))
        for l, s in enumerate(st["score_stds"][:n_layers]):
            scale(out, l, math.sqrt(target / max(s, 1e-6)))
    return out


def perceiver_weights(w, run, prefix="conditioning_perceiver.", inner=512, target=20.0):
    """Perceiver attention with peaked scores: to_q and the k half of to_kv (rows [0, inner)) scaled; run(w) runs the oracle"""
    depth = 0
    while f"{prefix}layers.{depth}.0.to_q.weight" in w:
        depth += 1

    def scale(ww, l, alpha):
        p = f"{prefix}layers.{l}.0."
        _put(ww, p + "to_q.weight", ww[p + "to_q.weight"].double().cpu() * alpha)
        kv = ww[p + "to_kv.weight"].double().cpu().clone()
        kv[:inner] *= alpha
        _put(ww, p + "to_kv.weight", kv)
    return _calibrate(w, run, depth, scale, target)


def hubert_weights(w, cfg, run, prefix="", target=20.0):
    """ContentVec self-attention with peaked scores: q_proj and k_proj (weights and biases) scaled; run(w) runs the oracle"""
    def scale(ww, l, alpha):
        p = f"{prefix}encoder.layers.{l}.self_attn."
        for n in ("q_proj.weight", "q_proj.bias", "k_proj.weight", "k_proj.bias"):
            _put(ww, p + n, ww[p + n].double().cpu() * alpha)
    return _calibrate(w, run, cfg["layers"], scale, target)


def dc_audio(wav, dc=0.5, ac=0.03, flat=(4000, 6000), level=0.01):
    """ContentVec input with a DC offset: the signal scaled by `ac` on top of `dc` (the first conv layer's channels then have a
    |mean| / std of a few hundred over time, what GroupNorm statistics see), and a stretch of constant non-zero samples (not padding:
    wav != 0)"""
    x = wav * ac + dc
    x[..., flat[0]:flat[1]] = dc + level
    return x


def round_bf16(w):
    """the matrices a bf16-weights context rounds at bind time (include/genvc_hip.h: weight_dtype)"""
    out = dict(w)
    for k, v in w.items():
        if k.endswith(("attn.c_attn.weight", "attn.c_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")) or k == "mel_head.weight":
            out[k] = v.to(torch.bfloat16).to(v.dtype)
    return out


# ---------------------------------------------------------------------------
# statistics of an oracle run
# ---------------------------------------------------------------------------

@contextlib.contextmanager
def record():
    """collect LayerNorm / GroupNorm input statistics and softmax score statistics of the oracle calls made inside the block"""
    st = dict(ln_ratios=[], max_abs=0.0, score_stds=[], spread=0.0, frac88=[], gn_ratio=0.0)
    ln0, gn0, sm0, tsm0 = F.layer_norm, F.group_norm, torch.softmax, torch.Tensor.softmax

    def ln(x, shape, *a, **kw):
        xd = x.detach().double()
        m = xd.mean(-1)
        s = xd.std(-1, unbiased=False).clamp_min(1e-30)
        st["ln_ratios"].append(float((m.abs() / s).median()))
        st["max_abs"] = max(st["max_abs"], float(xd.abs().max()))
        return ln0(x, shape, *a, **kw)

    def gn(x, groups, *a, **kw):
        xd = x.detach().double().reshape(x.shape[0], groups, -1)
        r = xd.mean(-1).abs() / xd.std(-1, unbiased=False).clamp_min(1e-30)
        st["gn_ratio"] = max(st["gn_ratio"], float(r.max()))
        return gn0(x, groups, *a, **kw)

    def note(s):
        sd = s.detach().double()
        fin = sd > -1e30
        if bool(fin.any()):
            hi = torch.where(fin, sd, torch.full_like(sd, -float("inf"))).amax(-1)
            lo = torch.where(fin, sd, torch.full_like(sd, float("inf"))).amin(-1)
            rng = hi - lo
            st["spread"] = max(st["spread"], float(rng.max()))
            st["frac88"].append(float((rng > 88.0).double().mean()))
            st["score_stds"].append(float(sd[fin].std()))

    def sm(s, dim=None, *a, **kw):
        note(s)
        return sm0(s, dim, *a, **kw)

    def tsm(self, dim=None, *a, **kw):
        note(self)
        return tsm0(self, dim, *a, **kw)

    F.layer_norm, F.group_norm, torch.softmax, torch.Tensor.softmax = ln, gn, sm, tsm
    try:
        yield st
    finally:
        F.layer_norm, F.group_norm, torch.softmax, torch.Tensor.softmax = ln0, gn0, sm0, tsm0


def summary(st):
    import statistics
    # (final_norm reads ln_f's output: one LayerNorm input in six of a 2-layer GPT is centred by construction, hence the median)
    return dict(ln_ratio=statistics.median(st["ln_ratios"]) if st["ln_ratios"] else 0.0,
                max_abs=st["max_abs"], spread=st["spread"],
                score_std=statistics.median(st["score_stds"]) if st["score_stds"] else 0.0,
                frac88=max(st["frac88"]) if st["frac88"] else 0.0, gn_ratio=st["gn_ratio"])


def check_regime(preset, st, what=""):
    """assert that an oracle run really entered the preset's regime; returns the summary"""
    s = summary(st)
    print(f"regime {what} {preset}: " + ", ".join(f"{k} {v:.3g}" for k, v in s.items()))
    for key, lo in REGIMES.get(preset, {}).items() if isinstance(preset, str) else ():
        assert s[key] >= lo, f"{what} preset {preset} stayed tame: {key} = {s[key]:.3g} < {lo}"
    return s


# ---------------------------------------------------------------------------
# the tolerance rule
# ---------------------------------------------------------------------------

def maxdev(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def yardstick(name, kern, ref64, ref32, kern_tame, ref64_tame):
    """the kernel's largest deviation from float64 must stay within max(8x the float32 oracle's own deviation, 4x the kernel's
    deviation on the default weights of the same shape and seed) + 1e-6 max|ref|.  Prints the three numbers; returns the bound."""
    dk = maxdev(kern, ref64)
    d32 = maxdev(ref32, ref64)
    dt = maxdev(kern_tame, ref64_tame)
    bound = max(8.0 * d32, 4.0 * dt) + 1e-6 * float(ref64.abs().max())
    print(f"{name}: kernel {dk:.3e}  fp32 oracle {d32:.3e}  kernel on default weights {dt:.3e}  bound {bound:.3e}")
    assert dk <= bound, f"{name}: kernel deviation from float64 {dk:.3e} > bound {bound:.3e} (fp32 oracle {d32:.3e}, default weights {dt:.3e})"
    return bound


def greedy_agrees(name, logits, ref64, bound, min_frac=0.5):
    """argmax of the kernel's logits == argmax of float64 wherever the float64 top-1 / top-2 margin is >= 10x the bound;
    most rows must qualify.  logits / ref64: [..., V]"""
    k = logits.detach().cpu().double().reshape(-1, logits.shape[-1])
    r = ref64.detach().cpu().double().reshape(-1, ref64.shape[-1])
    top = r.topk(2, -1)[0]
    ok = (top[:, 0] - top[:, 1]) >= 10.0 * bound
    frac = float(ok.double().mean())
    print(f"{name}: {int(ok.sum())}/{ok.numel()} rows with a margin >= 10x the bound")
    assert frac >= min_frac, f"{name}: only {frac:.2f} of the rows have a top-1 / top-2 margin >= 10x the bound"
    assert torch.equal(k.argmax(-1)[ok], r.argmax(-1)[ok]), f"{name}: greedy ids differ from float64 at a clear margin"
