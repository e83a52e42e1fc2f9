"""Time the acoustic DVAE on the device: decode, eval-mode forward (reconstruct) and the acoustic tokeniser, full configuration.

    python scripts/time_dvae_decode.py [--iters 50] [--out profiles/dvae_decode_time.json]

decode: n = 141 codes (one 6 s segment) at B = 1 and B = 8, n = 24 (one 1 s chunk) at B = 1.  Every shape is warmed up, then timed with
device events around `iters` back-to-back calls, alternating in the same process with the comparator: the same decoder as eager
PyTorch-ROCm (F.embedding / F.interpolate / F.conv1d on the same weights).  No earlier implementation exists in this repository, so
the comparator is the yardstick.  Figures, not thresholds:
  * ms per call; launches per call (by the launch rule of csrc/dvae.hip + launch_gemm_cap: a GEMM below 128 output tiles splits K and
    adds an epilogue launch);
  * algorithmic GFLOP = 2 x 35,291,136 x B n (the reference's arithmetic: k = 3 taps on the upsampled signal) over the time, and its
    share of the 157.3 TFLOP/s fp32 MFMA peak -- the decoder is MFMA-bound: its 109 MB of weights are ~14 us at the HBM peak.
The engine call includes what DiscreteVAE.decode includes: the gather, every conv, both outputs' stores, and the synchronising read of
the out-of-range mark (`decode_nocheck` leaves that read out: launches only, one synchronisation per timing loop).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
from genvc_amd._lib import check, lib, ptr, stream      # noqa: E402
from genvc_amd.layers.dvae import DiscreteVAE            # noqa: E402
from genvc_amd.utils import TorchMelSpectrogram          # noqa: E402

MACS_PER_CODE = 35_291_136
PEAK_TFLOPS = 157.3
DEV = "cuda"


def eager_decode(w, cfg, codes):
    x = F.embedding(codes, w["codebook.embed"].t()).permute(0, 2, 1)
    g = lambda n: (w[f"decoder.{n}.weight"], w[f"decoder.{n}.bias"])
    x = F.conv1d(x, *g("0"))
    idx = 1
    for _ in range(cfg["num_resnet_blocks"]):
        h = F.relu(F.conv1d(x, *g(f"{idx}.net.0"), padding=1))
        h = F.relu(F.conv1d(h, *g(f"{idx}.net.2"), padding=1))
        x = F.conv1d(h, *g(f"{idx}.net.4")) + x
        idx += 1
    for _ in range(cfg["num_layers"]):
        x = F.relu(F.conv1d(F.interpolate(x, scale_factor=2, mode="nearest"), *g(f"{idx}.0.conv"), padding=1))
        idx += 1
    return F.conv1d(x, *g(str(idx))), x


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def gemm_launches(M, N, K, batch):
    tiles = -(-M // 64) * -(-N // 64) * batch
    if tiles < 128:
        sk = min(-(-192 // tiles), max(K // 128, 1), 16)
        return 2 if sk > 1 else 1
    return 1


def decode_launches(cfg, B, n, pre_out=True):
    inner = cfg["hidden_dim"] * 2 ** (cfg["num_layers"] - 1)
    k = 2                                                                   # gather, its padding rows
    k += gemm_launches(n, inner, cfg["codebook_dim"], B) + 1                # 1x1 in, padding rows
    for _ in range(cfg["num_resnet_blocks"]):
        k += 2 * gemm_launches(n, inner, 3 * inner, B) + 1 + gemm_launches(n, inner, inner, B)
    ci, T = inner, n
    for i in range(cfg["num_layers"]):
        co = cfg["hidden_dim"] * 2 ** (cfg["num_layers"] - 1 - i)
        k += gemm_launches(T, co, 2 * ci, 2 * B) + 1                        # both phases in one batched GEMM, padding rows
        ci, T = co, 2 * T
    return k + (1 if pre_out else 0) + 1                                    # channel-major copy of the pre-output, last conv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = dict(gcfg.DEFAULT_ACOUSTIC_DVAE)
    m = DiscreteVAE(channels=cfg["num_channels"], num_tokens=cfg["num_tokens"], codebook_dim=cfg["codebook_dim"],
                    hidden_dim=cfg["hidden_dim"], num_resnet_blocks=cfg["num_resnet_blocks"], kernel_size=cfg["kernel_size"],
                    num_layers=cfg["num_layers"], positional_dims=1, use_transposed_convs=False, with_decoder=True)
    w = synth.make_weights(12, synth.dvae_full_weight_spec(cfg, codebook_scale=0.05), device=DEV)
    m.load_state_dict(w, strict=True)
    m.to(DEV).eval().bind(max_batch=8, max_frames=576)
    eng = m._engine
    res = dict(device=torch.cuda.get_device_name(0), iters=args.iters, decode=[], peak_tflops=PEAK_TFLOPS)
    with torch.inference_mode():
        for B, n in ((1, 141), (8, 141), (1, 24)):
            codes = synth.integers(5, f"time_codes_{B}_{n}", (B, n), cfg["num_tokens"]).to(DEV)
            c32 = codes.int().contiguous()
            out = torch.empty(B, 80, 4 * n, device=DEV)
            pre = torch.empty(B, cfg["hidden_dim"], 4 * n, device=DEV)

            def nocheck():
                check(lib().gvc_dvae_decode(eng._h, ptr(c32), B, n, ptr(out), ptr(pre), stream()), "decode")
            ref_out, _ = eager_decode(w, cfg, codes)
            err = float((m.decode(codes)[0] - ref_out).abs().max())
            t = {}
            for rnd in range(2):                        # alternate: engine, comparator, engine, comparator
                t.setdefault("decode", []).append(timed(lambda: m.decode(codes), args.iters))
                t.setdefault("decode_nocheck", []).append(timed(nocheck, args.iters))
                t.setdefault("eager", []).append(timed(lambda: eager_decode(w, cfg, codes), args.iters))
            gflop = 2.0 * MACS_PER_CODE * B * n / 1e9
            row = dict(B=B, n=n, max_abs_diff_vs_eager=err, launches=decode_launches(cfg, B, n), gflop=gflop)
            for k, v in t.items():
                ms = min(v)
                row[k + "_ms"] = ms
                row[k + "_ms_rounds"] = v
                row[k + "_tflops"] = gflop / ms
                row[k + "_share_of_peak"] = gflop / ms / PEAK_TFLOPS
            res["decode"].append(row)
            print(json.dumps(row))
        # eval-mode forward (encode -> VQ -> decode -> two losses) on one 6 s segment, and the acoustic tokeniser at 6 s
        feat = synth.uniform(5, "time_feat", (1, 80, 564), 1.0).to(DEV)
        res["reconstruct_1x564_ms"] = timed(lambda: eng.reconstruct(feat), args.iters)
        mel_fn = TorchMelSpectrogram(filter_length=1024, hop_length=256, win_length=1024, sampling_rate=24000, mel_fmin=0, mel_fmax=8000,
                                     n_mel_channels=80)
        wav = synth.synth_audio(5, "time_wav", 144000).to(DEV)
        res["tokeniser_6s_ms"] = timed(lambda: m.get_codebook_indices(mel_fn(wav)), args.iters)
        res["tokeniser_6s_codes"] = int(m.get_codebook_indices(mel_fn(wav)).shape[1])
    print(json.dumps({k: v for k, v in res.items() if k != "decode"}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
