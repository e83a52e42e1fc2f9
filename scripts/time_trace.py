"""Time the trace pass (GPT.trace / gvc_gpt_trace) next to the existing latent re-pass (GPT.forward(return_latent=True)) of the same
prompt and codes, in one process, in alternating rounds.

    python scripts/time_trace.py [--rounds 7] [--iters 5] [--out profiles/trace_time.json]

Shapes: the tiny dims (2 layers, d 256, 4 x 64; B 2, T 67) and the full depth and width (30 layers, d 1024) with the model's own
4 heads of 256 and with 16 heads of 64, T = 110 (13 content codes, 63 acoustic codes), B 1 and 5.  Per shape: milliseconds per call
(CUDA events around `iters` calls, the median over the rounds; every round times every variant once, in turn) of the re-pass and of
the trace with attentions / hidden states / alignment on and off, the ratio to the re-pass and the bytes each output writes.
Not a test and not bench.py.  Numbers for DESIGN.md section 4.23.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
from genvc_amd.layers.gpt import GPT      # noqa: E402

SHAPES = [
    ("tiny_b2", gcfg.TINY_MODEL_ARGS, 2, 9, 24),
    ("full_4x256_b1", gcfg.DEFAULT_MODEL_ARGS, 1, 13, 63),
    ("full_4x256_b5", gcfg.DEFAULT_MODEL_ARGS, 5, 13, 63),
    ("full_16x64_b1", dict(gcfg.DEFAULT_MODEL_ARGS, gpt_n_heads=16), 1, 13, 63),
    ("full_16x64_b5", dict(gcfg.DEFAULT_MODEL_ARGS, gpt_n_heads=16), 5, 13, 63),
]
VARIANTS = {                    # (output_attentions, output_hidden_states, alignment)
    "trace_attentions": (True, False, False),
    "trace_hidden": (False, True, False),
    "trace_alignment": (False, False, True),
    "trace_all": (True, True, True),
}


def once(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def run_shape(name, model_args, B, Tc, n, rounds, iters, models):
    dims = gcfg.gpt_dims(model_args)
    d, L, H = dims["d_model"], dims["n_layer"], dims["n_head"]
    dev = "cuda"
    key = (L, d, H)
    if key not in models:
        for old in models.values():            # one full-size context at a time
            old.engine.close()
        models.clear()
        m = GPT(layers=L, model_dim=d, heads=H, max_text_tokens=model_args["gpt_max_text_tokens"],
                max_mel_tokens=model_args["gpt_max_audio_tokens"], max_prompt_tokens=model_args["gpt_max_prompt_tokens"])
        m.load_state_dict(synth.make_weights(3, synth.gpt_weight_spec(dims)), strict=False)
        models[key] = m.to(dev).eval().init_gpt_for_inference(max_slots=8, max_rows=4096)
    m = models[key]
    text = synth.integers(3, "t", (B, Tc), 256).to(dev)
    codes = synth.integers(3, "c", (B, n), 1024).to(dev)
    cond = synth.uniform(3, "cond_latents", (B, 32, d), 1.0).to(dev)
    tl, wl = torch.full((B,), Tc), torch.full((B,), n * 1024)
    prefix = m.engine.prefix_embeddings(cond, text.int())
    slots = torch.arange(B, device=dev, dtype=torch.int32)
    lengths = torch.full((B,), n, dtype=torch.int32)
    fns = {"repass": lambda: m(text, tl, codes, wl, cond_latents=cond, return_latent=True)}
    for v, (at, hs, al) in VARIANTS.items():
        fns[v] = (lambda at=at, hs=hs, al=al: m.engine.trace(slots, prefix, codes.int(), lengths, 32, output_attentions=at,
                                                             output_hidden_states=hs, alignment=al))
    for fn in fns.values():                     # warm-up: every variant's kernels and allocations
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(once(fn, iters))
    P = 32 + Tc + 2
    T = P + n
    med = {k: statistics.median(v) for k, v in times.items()}
    res = dict(shape=name, layers=L, d_model=d, heads=H, B=B, T=T, repass_rows_per_item=T + 5,
               ms={k: round(v, 4) for k, v in med.items()},
               spread_ms={k: round(max(v) - min(v), 4) for k, v in times.items()},
               ratio_to_repass={k: round(med[k] / med["repass"], 3) for k in VARIANTS},
               bytes=dict(attentions=4 * L * B * H * T * T, hidden_states=4 * (L + 1) * B * T * d, alignment=4 * B * n * Tc,
                          alignment_scratch=4 * B * H * T * T))
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_trace.py measures on the GPU"
    models, out = {}, []
    for name, model_args, B, Tc, n in SHAPES:
        out.append(run_shape(name, model_args, B, Tc, n, args.rounds, args.iters, models))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(rounds=args.rounds, iters=args.iters, shapes=out), f, indent=1)


if __name__ == "__main__":
    main()
