"""weight_dtype 3 ("bf16_act") against weight_dtype 4 ("bf16_mfma") on the multi-row passes of the GPT, in one process:

    python scripts/time_bf16_mfma.py [out.json]

Per mode: bench.stage_times of the 8-stream workload, and CUDA-event times of the 8 x 48-row first prefill, the 8 x 16-row cached chunk
prefill, the 5 x 110-row prefill and a 5 x 141-code latent re-pass.  Then the GEMM probe (variant 1: fp32 strip kernel, variant 3:
bf16 strip kernel) at M = 128, 384, 550 for the four full-size projections.  A tree without the mode reports "bf16_act" only."""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from genvc_amd import _lib, synth  # noqa: E402

DEV = "cuda"


def shapes(wl, reps=10):
    eng, dims, dev = wl.eng, wl.dims, wl.dev
    d = dims["d_model"]
    out = {}

    def prefix(B, Tc, seed):
        cond = synth.uniform(seed, "c", (B, 32, d), 1.0).to(dev)
        return eng.prefix_embeddings(cond, synth.integers(seed, "k", (B, Tc), 256).to(dev).int())

    s8, s5 = torch.arange(8, device=dev, dtype=torch.int32), torch.arange(5, device=dev, dtype=torch.int32)
    p8, p5 = prefix(8, 13, 1), prefix(5, 75, 2)
    out["prefill_8x48_ms"] = bench._timed(lambda: eng.prefill(s8, p8, want_outputs=False), reps)
    eng.prefill(s8, p8, want_outputs=False)
    out["prefill_cached_8x16_ms"] = bench._timed(lambda: eng.prefill(s8, p8, want_outputs=False, n_cached=32), reps)
    out["prefill_5x110_ms"] = bench._timed(lambda: eng.prefill(s5, p5, want_outputs=False), reps)
    gen = synth.integers(3, "g", (5, 141), 1024).to(dev).int()
    out[f"latents_5x{p5.shape[1] + 141 + 5}_ms"] = bench._timed(lambda: eng.latents(s5, p5, gen), reps)
    return out


def probe(iters=20):
    out = {}
    g = torch.Generator().manual_seed(0)
    for name, (N, K) in (("c_attn", (3072, 1024)), ("attn_c_proj", (1024, 1024)), ("c_fc", (4096, 1024)), ("mlp_c_proj", (1024, 4096))):
        W = (torch.randn(N, K, generator=g) * 0.05).to(DEV)
        b = torch.randn(N, generator=g).to(DEV)
        for M in (128, 384, 550):
            A = torch.randn(M, K, generator=g).to(DEV)
            o = torch.empty(M, N, device=DEV)
            for variant in (1, 3):
                us = C.c_float(0)
                rc = _lib.lib().gvc_gemm_probe(variant, _lib.ptr(A), _lib.ptr(W), _lib.ptr(b), _lib.ptr(o), M, N, K, 8, iters, C.byref(us),
                                               _lib.stream())
                out[f"{name}_M{M}_variant{variant}_us"] = us.value if rc == 0 else None
    return out


def main():
    res = {"device": torch.cuda.get_device_name(0), "modes": {}}
    for mode in ("bf16_act", "bf16_mfma"):
        try:
            wl = bench.Workload(DEV, 0, 8, mode, max_slots=8)
        except KeyError:
            res["modes"][mode] = None           # a tree without the mode
            continue
        bench.warm_up_model(wl)
        wl.utterance(0)
        torch.cuda.synchronize()
        runs = [bench.stage_times(wl) for _ in range(3)]
        res["modes"][mode] = {"stage_times_ms": runs[-1], "utterance_total_ms_3_runs": [r["total"] for r in runs], **shapes(wl)}
        del wl
        torch.cuda.empty_cache()
    res["probe"] = probe()
    line = json.dumps(res)
    print(line)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
