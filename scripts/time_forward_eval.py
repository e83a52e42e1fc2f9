"""Time the evaluation pass of GPT.forward at the full model (30 x 1024, 4 heads of 256) next to the equal-length return_latent re-pass
of the same rows: 8 items x (32 conditioning + 152 text + 155 code) rows.

    python scripts/time_forward_eval.py [--iters 10] [--warmup 3]

Prints one JSON line: milliseconds per call (CUDA events, mean over the iterations), the algorithmic FLOPs of each call and the fraction
of the fp32 MFMA peak (157.3 TFLOP/s) they amount to.  Numbers for DESIGN.md section 4.20.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
from genvc_amd.layers.gpt import GPT, forward_eval_prepare      # noqa: E402

PEAK = 157.3e12


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    a = gcfg.DEFAULT_MODEL_ARGS
    dims = gcfg.gpt_dims(a)
    d, L, B, n_text, n_codes = dims["d_model"], dims["n_layer"], 8, 150, 150
    dev = "cuda"
    m = GPT(layers=L, model_dim=d, heads=a["gpt_n_heads"], max_text_tokens=a["gpt_max_text_tokens"],
            max_mel_tokens=a["gpt_max_audio_tokens"], max_prompt_tokens=a["gpt_max_prompt_tokens"])
    m.load_state_dict(synth.make_weights(3, synth.gpt_weight_spec(dims)), strict=False)
    m = m.to(dev).eval().init_gpt_for_inference(max_slots=B, max_rows=4096)
    text = synth.integers(3, "t", (B, n_text), 256).to(dev)
    codes = synth.integers(3, "c", (B, n_codes), 1024).to(dev)
    cond = synth.uniform(3, "cond_latents", (B, 32, d), 1.0).to(dev)
    full_t, full_w = torch.full((B,), n_text), torch.full((B,), n_codes * 1024)
    rag_t = torch.tensor([150, 20, 97, 150, 64, 131, 8, 113])
    rag_w = torch.tensor([150, 31, 88, 140, 150, 12, 77, 101]) * 1024 - 300
    prep = forward_eval_prepare(text, rag_t, codes, rag_w)
    Lt, Lm = prep["text_ids"].shape[1], prep["code_ids"].shape[1]
    T = 32 + Lt + Lm
    assert (Lt, Lm) == (152, 155)
    slots = torch.arange(B, device=dev, dtype=torch.int32)
    ti, ci, km = prep["text_ids"].to(dev).int(), prep["code_ids"].to(dev).int(), prep["key_mask"].to(dev, torch.uint8)
    lat = m.engine.forward_rows(slots, cond, ti, ci, km)
    tt, mt = prep["text_targets"].reshape(-1).to(dev).int(), prep["mel_targets"].reshape(-1).to(dev).int()
    lt_rows, lm_rows = lat[:, :Lt].reshape(B * Lt, d).contiguous(), lat[:, Lt:].reshape(B * Lm, d).contiguous()

    def heads():
        m.engine.head_xent(lt_rows, "text", tt)
        m.engine.head_xent(lm_rows, "mel", mt)
    res = dict(rows=B * T, rows_per_item=T,
               repass_ms=timed(lambda: m(text, full_t, codes, full_w, cond_latents=cond, return_latent=True), args.warmup, args.iters),
               rows_unmasked_ms=timed(lambda: m.engine.forward_rows(slots, cond, ti, ci, None), args.warmup, args.iters),
               rows_masked_ms=timed(lambda: m.engine.forward_rows(slots, cond, ti, ci, km), args.warmup, args.iters),
               heads_ms=timed(heads, args.warmup, args.iters),
               forward_ms=timed(lambda: m(text, rag_t, codes, rag_w, cond_latents=cond), args.warmup, args.iters))
    # algorithmic FLOPs: 24 d^2 per row and layer in the four projections, 2 T^2 d per item and layer in the causal attention
    # (Q K^T and P V over half the square), 2 d V per head row
    stack = L * (B * T * 24 * d * d + B * 2 * T * T * d)
    head_flops = 2 * d * (B * Lt * 258 + B * Lm * 1026)
    res.update(stack_gflop=stack / 1e9, heads_gflop=head_flops / 1e9,
               repass_peak_fraction=stack / (res["repass_ms"] * 1e-3) / PEAK,
               rows_masked_peak_fraction=stack / (res["rows_masked_ms"] * 1e-3) / PEAK,
               forward_peak_fraction=(stack + head_flops) / (res["forward_ms"] * 1e-3) / PEAK)
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in res.items()}))


if __name__ == "__main__":
    main()
