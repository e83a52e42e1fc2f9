"""Time one vocoder eval_step worth of work on the device -- MSD + MPD on 2 B waveforms with their reductions, the criteria and the mel
loss -- against eager PyTorch on the same GPU running the oracle's modules (tests/vocoder_eval_oracle.py).

    python scripts/time_vocoder_eval.py [--iters 10] [--batch 8] [--seconds 6] [--out profiles/vocoder_eval_time.json]

B = 8, 6 s of 24 kHz audio by default.  Every figure is the median of `--rounds` rounds of `iters` back-to-back calls between device
events after a warm-up, engine and comparator alternating in one process.  Per layer: gvc_disc_time_layer (the layer's launch alone on
the arena's contents) with its MACs and, for the matrix-core layers, the share of the 157.3 TFLOP/s fp32 MFMA peak.  Figures, not
thresholds."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vocoder_eval_oracle as VO                                   # noqa: E402
from genvc_amd.layers import hifigan_loss as HL                    # noqa: E402
from genvc_amd.layers.hifigan import MultiPeriodDiscriminator, MultiScaleDiscriminator      # noqa: E402

PEAK_TFLOPS = 157.3
DEV = "cuda"


def timed(fn, iters, rounds):
    for _ in range(2):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, T = args.batch, int(args.seconds * 24000)
    cfg = VO.mpd_cfg(1)
    w_msd, w_mpd = VO.msd_weights(device=DEV), VO.mpd_weights(cfg, device=DEV)
    msd = MultiScaleDiscriminator()
    msd.load_state_dict(w_msd, strict=True)
    msd.to(DEV).eval().bind(max_batch=B, max_samples=T)
    mpd = MultiPeriodDiscriminator(cfg["mpd_reshapes"], 1, False)
    mpd.load_state_dict(w_mpd, strict=True)
    mpd.to(DEV).eval().bind(max_batch=B, max_samples=T)
    y, g = VO.wav_pair(7, B, T, DEV)
    crit, mel = HL.discriminator_criterion(), HL.mel_criterion(VO.MEL_CFG)
    basis = torch.from_numpy(VO.slaney_filterbank(24000, 1024, 100, 0, 12000)).to(DEV)

    def device_step():
        total = 0.0
        for d in (msd, mpd):
            y_r, y_g, _, _ = d(y, g)
            total = total + float(crit(y_r, y_g)[0])
        return total, float(mel(y, g))

    def eager_step():
        total = 0.0
        for fn in (lambda: VO.msd(w_msd, y, g), lambda: VO.mpd(w_mpd, cfg["mpd_reshapes"], y, g)):
            d_r, d_g, _, _ = fn()
            total = total + float(VO.discriminator_criterion(d_r, d_g)[0])
        a = VO.extract_mel_features(y.reshape(B, T), basis=basis)
        b = VO.extract_mel_features(g.reshape(B, T), basis=basis)
        return total, float(torch.nn.functional.l1_loss(a, b) * 45)

    res = dict(device=torch.cuda.get_device_name(0), B=B, T=T, iters=args.iters, rounds=args.rounds, peak_tflops=PEAK_TFLOPS)
    with torch.inference_mode():
        res["device_losses"], res["eager_losses"] = device_step(), eager_step()
        t = {}
        for name, fn in (("device_step", device_step), ("eager_step", eager_step),
                         ("device_msd", lambda: msd(y, g)), ("eager_msd", lambda: VO.msd(w_msd, y, g)),
                         ("device_mpd", lambda: mpd(y, g)), ("eager_mpd", lambda: VO.mpd(w_mpd, cfg["mpd_reshapes"], y, g)),
                         ("device_mel", lambda: mel(y, g))):
            t[name + "_ms"], t[name + "_ms_rounds"] = timed(fn, args.iters, args.rounds)
            print(name, f"{t[name + '_ms']:.3f} ms", flush=True)
        res.update(t)
        layers = []
        for tag, d in (("msd", msd), ("mpd", mpd)):
            eng = d._engine
            d(y, g)
            for i in range(eng.n_sub):
                cin = 1
                for l in range(eng.n_layers):
                    fm = eng.layer(i, l, B, T)
                    conv = d.discriminators[i].conv_post if l == eng.n_layers - 1 else d.discriminators[i].convs[l]
                    wt = conv.weight_orig if hasattr(conv, "weight_orig") else conv.weight_v
                    macs = fm.numel() * wt[0].numel()                  # outputs x (C_in / groups x taps)
                    us = statistics.median(eng.time_layer(i, l, B, T, args.iters) for _ in range(args.rounds))
                    row = dict(disc=tag, sub=i, layer=l, shape=list(fm.shape), weight=list(wt.shape), gmac=macs / 1e9, us=us,
                               tflops=2.0 * macs / us / 1e6, out_gbytes_per_s=fm.numel() * 4 / us / 1e3)
                    row["share_of_fp32_mfma_peak"] = row["tflops"] / PEAK_TFLOPS if 0 < l < eng.n_layers - 1 else None
                    layers.append(row)
                    cin = fm.shape[1]
        res["layers"] = layers
        for row in sorted(layers, key=lambda r: -r["gmac"])[:3]:
            print("widest:", json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "layers"}))


if __name__ == "__main__":
    main()
