"""Generate tests/golden/hifigan_v1.npz: the reference's HiFiGAN(resblock_type="1") (layers/hifigan.py:28-117, 160-233) on synthetic
weights, in fp32 and fp64.

Runs only where the reference checkout is present; nothing of it is copied -- its class is imported, loaded with genvc_amd.synth
weights (hifigan_weight_spec of a resblock_type "1" config) and called.  torchaudio, nnAudio and the other third-party modules that
file imports are absent and stubbed here; none of the stubs computes anything on this path.

    python scripts/make_hifigan_v1_golden.py [--reference /path/to/reference]

Per case of hifigan_v1_oracle.CASES (tag t):
  * `{t}_keys`: the reference module's state-dict key list;
  * `{t}_wav` [B,1,T * up]: its fp32 waveform;
  * `floor_{t}` = max(max|fp32 - fp64|, 2^-24 max|wav|): the second term is half an fp32 ulp of the largest sample;
  * `{t}_range`: (min, max) of the waveform, as printed.
The script asserts that the oracle restatement (tests/hifigan_v1_oracle.py) matches the reference within each floor, and that no
stored waveform is saturated or degenerate (1e-3 <= max|wav| <= 0.99).
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
import hifigan_v1_oracle as HO            # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def import_reference(path):
    sys.dont_write_bytecode = True

    def stub(name):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
        return sys.modules[name]

    ta = stub("torchaudio")
    for sub in ("transforms", "functional"):
        if not hasattr(ta, sub):
            setattr(ta, sub, stub("torchaudio." + sub))
    na = stub("nnAudio")
    if not hasattr(na, "features"):
        na.features = stub("nnAudio.features")
    stub("fsspec")
    stub("einops").__dict__.setdefault("rearrange", None)
    mpl = stub("matplotlib")
    if not hasattr(mpl, "pylab"):
        mpl.pylab = stub("matplotlib.pylab")
        mpl.use = lambda *a, **k: None
    lr = stub("librosa")
    if not hasattr(lr, "filters"):
        lr.filters = stub("librosa.filters")
    sys.path.insert(0, path)
    from layers import hifigan as H
    return H


@torch.inference_mode()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    args = ap.parse_args()
    H = import_reference(args.reference)
    out = dict(seed=HO.SEED)
    worst = 0.0
    for tag, cfg, B, T in HO.CASES:
        model = H.HiFiGAN(cfg["input_feat_dim"], cfg["upsample_initial_channel"], cfg["resblock_kernel_sizes"],
                          cfg["resblock_dilation_sizes"], cfg["upsample_rates"], cfg["upsample_kernel_sizes"], resblock_type="1")
        w = HO.weights(cfg)
        model.load_state_dict(w, strict=True)
        model.eval()
        x = HO.frames(HO.SEED, B, T, cfg["input_feat_dim"])
        y32 = model(x)
        o32 = HO.generator(w, cfg, x)
        y64 = model.double()(x.double())
        fl = HO.floor_of(y32, y64)
        err = float((y32.double() - o32.double()).abs().max())
        assert err <= fl, (tag, err, fl)
        worst = max(worst, err / fl)
        peak = float(y32.abs().max())
        assert 1e-3 <= peak <= 0.99, (tag, peak)
        out[f"{tag}_keys"] = np.array(list(model.state_dict().keys()))
        out[f"{tag}_wav"] = y32.numpy()
        out[f"floor_{tag}"] = np.float64(fl)
        out[f"{tag}_range"] = np.array([float(y32.min()), float(y32.max())], dtype=np.float32)
        print(f"{tag}: B={B} T={T} -> {tuple(y32.shape)} range [{float(y32.min()):.4f}, {float(y32.max()):.4f}] floor {fl:.3e} "
              f"oracle - reference {err:.3e}")
    path = os.path.join(GOLD, "hifigan_v1.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 900 * 1024, size
    print(f"hifigan_v1.npz: {len(out)} arrays, {size} bytes, oracle vs reference at most {worst:.2f} of a floor")


if __name__ == "__main__":
    main()
