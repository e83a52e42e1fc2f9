"""The streaming-size HiFi-GAN call (8 tokens -> 32 frames -> 8192 samples, B = 1) with ResBlock1: the full V1 generator
(upsample_initial_channel 256, rates 8 / 8 / 4, kernels 3 / 7 / 11, dilations 1 / 3 / 5) on the six-launches-per-stage path and on the
one-launch-per-conv fall-back of the same build (GVC_VOCODER_SMALL_CONV=0), with the ResBlock2 call of the default config beside them.

    python scripts/time_hifigan_v1.py [--out profiles/hifigan_v1_time.json] [--reps 200]

Per variant: device time per call over `reps` back-to-back calls (device events), the isolated call (enqueue -> synchronized, as the
streaming loop issues it), the node count of the captured graph (its launches) and the stages on the one-round-trip kernel.  The
variants are timed in turn, three rounds, and the median round is kept.  Needs a GPU; nothing is asserted about the ratio."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                    # noqa: E402
from genvc_amd import config as gcfg, synth                      # noqa: E402
from genvc_amd.engine import HifiganEngine                       # noqa: E402

V1 = dict(gcfg.DEFAULT_VOCODER, **gcfg.V1_RESBLOCKS)


def engine(cfg, small_conv):
    """small_conv None: the default path; "0": GVC_VOCODER_SMALL_CONV=0 while the context is created (it is read there); the caller's
    own value of the variable is put back afterwards"""
    saved = os.environ.pop("GVC_VOCODER_SMALL_CONV", None)
    if small_conv is not None:
        os.environ["GVC_VOCODER_SMALL_CONV"] = small_conv
    try:
        eng = HifiganEngine(cfg, max_batch=2, max_frames=64)
    finally:
        os.environ.pop("GVC_VOCODER_SMALL_CONV", None)
        if saved is not None:
            os.environ["GVC_VOCODER_SMALL_CONV"] = saved
    eng.bind(synth.make_weights(5, synth.hifigan_weight_spec(cfg), device="cuda"))
    return eng


def time_call(eng, lat, reps):
    for _ in range(5):
        eng.forward_latents(lat, 4)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        eng.forward_latents(lat, 4)
    e1.record()
    torch.cuda.synchronize()
    t = 0.0
    for _ in range(reps):
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        eng.forward_latents(lat, 4)
        torch.cuda.synchronize()
        t += time.perf_counter() - h0
    return e0.elapsed_time(e1) / reps * 1e3, t / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_hifigan_v1.py needs a GPU"
    lat = synth.uniform(7, "lat", (1, 8, 1024), 1.0).cuda()
    variants = {"resblock1_small_conv": engine(V1, None), "resblock1_launch_per_conv": engine(V1, "0"),
                "resblock2_default": engine(gcfg.DEFAULT_VOCODER, None)}
    rounds = {k: [] for k in variants}
    for _ in range(3):
        for k, eng in variants.items():
            rounds[k].append(time_call(eng, lat, args.reps))
    res = {}
    for k, eng in variants.items():
        res[k] = dict(device_us_per_call=round(statistics.median(r[0] for r in rounds[k]), 2),
                      isolated_call_us=round(statistics.median(r[1] for r in rounds[k]), 2),
                      device_us_rounds=[round(r[0], 2) for r in rounds[k]], graph_nodes=eng.graph_nodes, lds_stages=eng.lds_stages)
    # the two ResBlock1 paths compute the same thing: how far apart are they
    a = variants["resblock1_small_conv"].forward_latents(lat, 4)
    b = variants["resblock1_launch_per_conv"].forward_latents(lat, 4)
    torch.cuda.synchronize()
    out = dict(call="B=1, 8 latents -> 32 frames -> 8192 samples", reps=args.reps, device=torch.cuda.get_device_name(0), variants=res,
               launch_per_conv_over_small_conv=round(res["resblock1_launch_per_conv"]["device_us_per_call"] /
                                                     res["resblock1_small_conv"]["device_us_per_call"], 3),
               max_abs_difference_between_paths=float((a - b).abs().max()), max_abs_wav=float(a.abs().max()))
    print(json.dumps(out, indent=1))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
