"""Generate tests/golden/vocoder_eval.npz: the reference's MultiScaleDiscriminator, MultiPeriodDiscriminator (layers/hifigan.py) and
the criteria of layers/hifigan_loss.py on synthetic weights and waveforms, in eval mode.

Runs only where the reference checkout is present; nothing of it is copied -- its classes are imported, loaded with genvc_amd.synth
weights (msd_weight_spec, mpd_weight_spec) and called.  torchaudio, nnAudio and librosa are absent and stubbed here; the one stub
that computes is librosa.filters.mel, which is tests/vocoder_eval_oracle.slaney_filterbank: THE FILTERBANK IS THE ONE STAGE NOTHING
HERE CAN PIN (torch.stft, the padding, the magnitude, the log are the reference's own calls).

    python scripts/make_vocoder_eval_golden.py [--reference /path/to/reference]

Per case of vocoder_eval_oracle.CASES (tag t) and discriminator D in (msd, mpd):
  * `{t}_{D}_keys`: the state dict's key list;  `{t}_{D}_dr{i}` / `_dg{i}`: every sub-discriminator's logits in full;
  * `{t}_{D}_fr{i}_{l}` / `_fg{i}_{l}`: the feature maps, sub-sampled (vocoder_eval_oracle.subsample);
  * `{t}_{D}_fmean` [n_sub, n_layers]: mean|f_r - f_g|;  `_disc`, `_rl`, `_gl`, `_gen`, `_genl`, `_feat`: the criteria;
  * `{t}_{D}_w{i}_{l}`: the first 64 entries of three folded weights (a spectral-normed one where there is one);
  * case a: `mel_feat` (item 0, real) and `mel_loss`.
Every quantity q has `floor_q` = max(max|fp32 - fp64| of the reference run in both precisions, 2^-24 max|q|): the second term is half
an fp32 ulp of the largest entry, below which no fp32 result can be told from the fp64 one.  `floor_.._fmean` is an array, one floor per
(sub-discriminator, layer): a mean over a map moves by at most max|df_r| + max|df_g| when the maps move, so an entry's floor is also
at least the sum of its two (whole) maps' floors -- a conv_post map of a few dozen elements has no averaging to hide behind, and one
maximum over all entries (which collapses to the half-ulp term) is no floor for it.  For the two mel quantities the fp64 side
is the oracle's restatement (the reference's extractor pins its window and filterbank to fp32 tensors).  The script asserts that the
oracle restatement matches the reference within each floor.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from genvc_amd import synth               # noqa: E402
import vocoder_eval_oracle as VO          # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def import_reference(path):
    sys.dont_write_bytecode = True

    def stub(name, **attrs):
        try:
            __import__(name)
            return sys.modules[name]
        except ImportError:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
            return m

    ta = stub("torchaudio")
    for sub in ("transforms", "functional"):
        if not hasattr(ta, sub):
            setattr(ta, sub, stub("torchaudio." + sub))
    na = stub("nnAudio")
    if not hasattr(na, "features"):
        na.features = stub("nnAudio.features")
    stub("fsspec")
    mpl = stub("matplotlib")
    if not hasattr(mpl, "pylab"):
        mpl.pylab = stub("matplotlib.pylab")
        mpl.use = lambda *a, **k: None
    lr = stub("librosa")
    if not hasattr(lr, "filters"):
        lr.filters = stub("librosa.filters")
        lr.filters.mel = lambda sr, n_fft, n_mels, fmin, fmax: VO.slaney_filterbank(sr, n_fft, n_mels, fmin, fmax)
    sys.path.insert(0, path)
    from layers import hifigan as H
    from layers import hifigan_loss as HL
    return H, HL


def t2n(t):
    return t.detach().to(torch.float64).numpy() if t.dtype == torch.float64 else t.detach().numpy()


def run(model, HL, y, g):
    """every stored quantity of one discriminator at one precision -> {name: ndarray}"""
    d_r, d_g, f_r, f_g = model(y, g)
    q = {}
    run.full = [[(t2n(a), t2n(b)) for a, b in zip(fr, fg)] for fr, fg in zip(f_r, f_g)]       # the whole maps of this run (not stored)
    for i in range(len(d_r)):
        q[f"dr{i}"], q[f"dg{i}"] = t2n(d_r[i]), t2n(d_g[i])
        for l in range(len(f_r[i])):
            q[f"fr{i}_{l}"], q[f"fg{i}_{l}"] = t2n(VO.subsample(f_r[i][l])), t2n(VO.subsample(f_g[i][l]))
    q["fmean"] = np.array([[float(torch.mean(torch.abs(a - b))) for a, b in zip(fr, fg)] for fr, fg in zip(f_r, f_g)],
                          dtype=np.float64 if y.dtype == torch.float64 else np.float32)
    loss, rl, gl = HL.discriminator_criterion()(d_r, d_g)
    gen, genl = HL.generator_criterion()(d_g)
    q["disc"], q["rl"], q["gl"] = t2n(loss), np.array(rl), np.array(gl)
    q["gen"], q["genl"], q["feat"] = t2n(gen), np.array([float(v) for v in genl]), t2n(HL.feature_criterion()(f_r, f_g))
    return q


def oracle_run(fn, y, g):
    d_r, d_g, f_r, f_g = fn(y, g)
    q = {}
    for i in range(len(d_r)):
        q[f"dr{i}"], q[f"dg{i}"] = t2n(d_r[i]), t2n(d_g[i])
        for l in range(len(f_r[i])):
            q[f"fr{i}_{l}"], q[f"fg{i}_{l}"] = t2n(VO.subsample(f_r[i][l])), t2n(VO.subsample(f_g[i][l]))
    q["fmean"] = np.array([[float(v) for v in row] for row in VO.feature_means(f_r, f_g)])
    loss, rl, gl = VO.discriminator_criterion(d_r, d_g)
    gen, genl = VO.generator_criterion(d_g)
    q["disc"], q["rl"], q["gl"] = t2n(loss), np.array(rl), np.array(gl)
    q["gen"], q["genl"], q["feat"] = t2n(gen), np.array([float(v) for v in genl]), t2n(VO.feature_criterion(f_r, f_g))
    return q


def floor_of(a32, a64):
    a32, a64 = np.asarray(a32, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    return float(max(np.abs(a32 - a64).max(), 2.0 ** -24 * np.abs(a64).max()))


@torch.inference_mode()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    H, HL = import_reference(args.reference)
    out = dict(seed=VO.SEED)
    worst = 0.0
    for tag, B, T, mult in VO.CASES:
        y, g = VO.wav_pair(VO.SEED, B, T)
        cfg = VO.mpd_cfg(mult)
        for D in ("msd", "mpd"):
            if D == "msd":
                model, w = H.MultiScaleDiscriminator(), VO.msd_weights()
                fn = lambda a, b: VO.msd(w, a, b)                      # noqa: E731
            else:
                model = H.MultiPeriodDiscriminator(cfg["mpd_reshapes"], mult, False)
                w = VO.mpd_weights(cfg)
                fn = lambda a, b: VO.mpd(w, cfg["mpd_reshapes"], a, b)  # noqa: E731
            model.load_state_dict(w, strict=True)
            model.eval()
            out[f"{tag}_{D}_keys"] = np.array(list(model.state_dict().keys()))
            q32 = run(model, HL, y, g)
            o32 = oracle_run(fn, y, g)
            # three folded weights: the eval-mode forward leaves them in `.weight`
            for i, l in ((0, 1), (1, len(model.discriminators[1].convs) - 1), (len(model.discriminators) - 1, -1)):
                conv = model.discriminators[i].conv_post if l < 0 else model.discriminators[i].convs[l]
                name = f"discriminators.{i}." + ("conv_post" if l < 0 else f"convs.{l}")
                ll = len(model.discriminators[i].convs) if l < 0 else l
                fw = conv.weight.detach().reshape(-1)[:64].clone()
                assert torch.equal(fw, VO.folded(w, name).reshape(-1)[:64]), name
                out[f"{tag}_{D}_w{i}_{ll}"] = fw.numpy()
            model.double()
            full32 = run.full
            q64 = run(model, HL, y.double(), g.double())
            # mean|f_r - f_g| moves by at most max|df_r| + max|df_g| when the maps move (triangle inequality): entry by entry
            map_floor = np.array([[floor_of(a32, a64) + floor_of(b32, b64) for (a32, b32), (a64, b64) in zip(r32, r64)]
                                  for r32, r64 in zip(full32, run.full)])
            for k in q32:
                fl = floor_of(q32[k], q64[k])
                if k == "fmean":
                    fl = np.maximum(map_floor, np.maximum(np.abs(q32[k].astype(np.float64) - q64[k]), 2.0 ** -24 * np.abs(q64[k])))
                err = float(np.abs(np.asarray(q32[k], dtype=np.float64) - np.asarray(o32[k], dtype=np.float64)).max())
                assert err <= np.min(fl), (tag, D, k, err, fl)
                worst = max(worst, err / float(np.min(fl)))
                out[f"{tag}_{D}_{k}"] = np.asarray(q32[k], dtype=np.float32)
                out[f"floor_{tag}_{D}_{k}"] = np.asarray(fl, dtype=np.float64)
            print(f"{tag} {D}: B={B} T={T} disc {float(q32['disc']):.6f} gen {float(q32['gen']):.6f} feat {float(q32['feat']):.6f} "
                  f"logit range [{min(float(q32[k].min()) for k in q32 if k[:2] in ('dr', 'dg')):.3f}, "
                  f"{max(float(q32[k].max()) for k in q32 if k[:2] in ('dr', 'dg')):.3f}]")
        if tag == "a":
            mcfg = types.SimpleNamespace(**VO.MEL_CFG)
            feat = HL.extract_mel_features(y.squeeze(), mcfg)
            loss = HL.mel_criterion(mcfg)(y, g)
            o_feat, o_loss = VO.extract_mel_features(y.reshape(B, T)), VO.mel_criterion(y, g)
            f64, l64 = VO.extract_mel_features(y.reshape(B, T).double()), VO.mel_criterion(y.double(), g.double())
            for k, a, o, d in (("mel_feat", feat[0], o_feat[0], f64[0]), ("mel_loss", loss, o_loss, l64)):
                fl = floor_of(t2n(a), t2n(d))
                err = float((a.double() - o.double()).abs().max())
                assert err <= fl, (k, err, fl)
                out[k], out["floor_" + k] = t2n(a).astype(np.float32), np.float64(fl)
            print(f"mel: features {tuple(feat.shape)}, loss {float(loss):.6f} (floors {out['floor_mel_feat']:.2e} {out['floor_mel_loss']:.2e})")
    path = os.path.join(GOLD, "vocoder_eval.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 900 * 1024, size
    print(f"vocoder_eval.npz: {len(out)} arrays, {size} bytes, oracle vs reference at most {worst:.2f} of a floor")


if __name__ == "__main__":
    main()
