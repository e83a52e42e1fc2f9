"""Cost of contrastive search on one MI355X: full size (GenVC_small dims, synthetic weights), one item, a 48-row prompt
(32 conditioning latents + 13 content codes + 3), K in {2, 4, 8}, for 24 and ~300 steps so the growing context shows.

    python scripts/time_contrastive.py [--out profiles/contrastive_time.json] [--reps 5] [--steps 24 296]

ms_per_step: device time (events) of the contrastive_generate calls of one run -- prefill excluded, every step replayed from the warmed
graphs (eight steps per graph) -- divided by the steps; the median over `reps` runs.  The stop token is biased away (mel_head.bias[1025]
= -30) so every run takes all its steps.  For comparison the greedy loop of the same shape (generate, top_k = 1) is timed too."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402


def build_gpt(max_slots=8):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.DEFAULT_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    dims = gcfg.gpt_dims(a)
    w = synth.make_weights(1, synth.gpt_weight_spec(dims))
    w["mel_head.bias"][1025] = -30.0
    g.load_state_dict(w, strict=False)
    g.to("cuda")
    g.init_gpt_for_inference(max_slots=max_slots)
    return g, dims


def time_run(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    steps = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrastive_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, nargs="+", default=[24, 296])
    ap.add_argument("--ks", type=int, nargs="+", default=[2, 4, 8])
    args = ap.parse_args()
    from genvc_amd.engine import ContrastiveSearch
    g, dims = build_gpt()
    eng = g.engine
    d = dims["d_model"]
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    fake = g.compute_embeddings(cond, codes)
    prefix = g._prefix
    n0 = int(fake.shape[1])
    assert n0 == 48
    hi = n0 + max(args.steps)
    eng.warmup(1, hi, 1)
    eng.warmup_range(1, n0 + 1, hi, 1)
    for K in args.ks:
        eng.warmup_contrastive(1, K, hi)
    res = dict(device=torch.cuda.get_device_name(0), n0=n0, reps=args.reps, rows={})
    for n in args.steps:
        def greedy():
            st = g._start(fake, dict(do_sample=False, max_new_tokens=n))
            g._advance(st, n)
            return n
        ts = sorted(time_run(greedy)[0] for _ in range(args.reps))
        res["rows"][f"greedy_n{n}"] = dict(K=1, steps=n, ms_per_step=ts[len(ts) // 2] / n, ms_all=ts)
        for K in args.ks:
            slots = torch.arange(K, device="cuda", dtype=torch.int32)

            def run():
                cs = ContrastiveSearch(fake, K, n, 1025, dims["num_audio_tokens"], d, 0.6, 1.0, latents=True)
                eng.prefill_hidden(slots[::K].contiguous(), prefix, cs.hidden0)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                eng.contrastive_generate(slots, cs, n, max_keys=n0 + n)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1)
            ts = sorted(run() for _ in range(args.reps))
            res["rows"][f"K{K}_n{n}"] = dict(K=K, steps=n, ms_per_step=ts[len(ts) // 2] / n, ms_all=ts,
                                             variant=eng.decode_variant())
            print(f"K={K} n={n}: {ts[len(ts) // 2] / n:.3f} ms/step (variant {eng.decode_variant()})", flush=True)
        print(f"greedy n={n}: {res['rows'][f'greedy_n{n}']['ms_per_step']:.3f} ms/step (prefill included)", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: round(v["ms_per_step"], 4) for k, v in res["rows"].items()}))


if __name__ == "__main__":
    main()
