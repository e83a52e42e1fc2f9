"""Time TorchMelSpectrogram.invert (inverse mel scale + 64 Griffin-Lim iterations, csrc/griffinlim.hip) on a 10 s mel at B = 1 and
B = 8 against the oracle's loop (tests/griffinlim_oracle.py: torch.linalg.lstsq, torch.stft, torch.istft) run in eager PyTorch on the
same GPU.

    python scripts/time_griffinlim.py [--iters 5] [--rounds 5] [--seconds 10] [--n_iter 64] [--out profiles/griffinlim_time.json]

Every figure is the median of `--rounds` rounds of `iters` back-to-back calls between device events after a warm-up, engine and
comparator alternating in one process.  The kernel launches of one call are counted by the library (gvc_gl_launches).  Figures, not
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
import griffinlim_oracle as GO                                     # noqa: E402
from genvc_amd.utils import TorchMelSpectrogram                    # noqa: E402

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
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--n_iter", type=int, default=64)
    ap.add_argument("--sample_rate", type=int, default=24000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tm = TorchMelSpectrogram(sampling_rate=args.sample_rate)
    a = tm.args
    T = int(args.seconds * args.sample_rate)
    norms = tm.mel_norms.to(DEV)
    fb = GO.filterbank(a["n_fft"], a["sample_rate"], a["f_min"], a["f_max"], a["n_mels"]).to(DEV)
    res = dict(device=torch.cuda.get_device_name(0), seconds=args.seconds, sample_rate=args.sample_rate, n_fft=a["n_fft"], hop=a["hop"],
               win=a["win"], n_iter=args.n_iter, iters=args.iters, rounds=args.rounds, cases=[])
    with torch.inference_mode():
        for B in (1, 8):
            wav = torch.stack([GO.harmonic_noise_wav(90 + i, 1, T, args.sample_rate)[0] for i in range(B)]).to(DEV)
            mel = tm(wav)
            F = mel.shape[-1]
            tm.bind_invert(max_batch=B, max_frames=F)
            eng = tm._gl_engine
            init = eng.init_angles(0, B, F)

            def device_call():
                return tm.invert(mel, n_iter=args.n_iter, init_angles=init)

            S_dev = eng.inverse_mel(mel)
            try:                                        # torch.linalg.lstsq on the device needs a solver backend in the torch build
                GO.inverse_mel(mel, norms, fb)
                eager_lstsq = True
            except RuntimeError as e:
                eager_lstsq = False
                print(f"eager inverse mel not measured: {e}", flush=True)

            def eager_call():
                S = GO.inverse_mel(mel, norms, fb) if eager_lstsq else S_dev
                return GO.griffinlim(S, init, args.n_iter, a["n_fft"], a["hop"], a["win"])

            n0 = eng.launches()
            got = device_call()
            launches = eng.launches() - n0
            want = eager_call()
            S = S_dev
            case = dict(B=B, eager_includes_inverse_mel=eager_lstsq, frames=F, samples=int(got.shape[1]), launches_per_call=launches,
                        max_abs_diff_device_vs_eager=float((got - want).abs().max()), peak=float(want.abs().max()),
                        spectral_convergence_device=GO.spectral_convergence(got.cpu(), S.cpu(), a["n_fft"], a["hop"], a["win"]).tolist(),
                        spectral_convergence_eager=GO.spectral_convergence(want.cpu(), S.cpu(), a["n_fft"], a["hop"], a["win"]).tolist())
            runs = [("device", device_call), ("eager", eager_call), ("device_inverse_mel", lambda: eng.inverse_mel(mel))]
            if eager_lstsq:
                runs.append(("eager_inverse_mel", lambda: GO.inverse_mel(mel, norms, fb)))
            for name, fn in runs:
                case[name + "_ms"], case[name + "_ms_rounds"] = timed(fn, args.iters, args.rounds)
                print(f"B={B} {name}: {case[name + '_ms']:.3f} ms", flush=True)
            case["ffts_per_call"] = B * F * (2 * args.n_iter + 1)
            res["cases"].append(case)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
