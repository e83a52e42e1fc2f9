"""Decode loops with the logits processors on or off, for a per-kernel comparison under
`rocprofv3 --kernel-trace --stats -- python scripts/time_processors.py --proc on|off`: full-size synthetic weights, one 1 s segment
(13 content codes -> a 48-row prompt), 40 tokens per call, `reps` calls each of the greedy sampler (k_sample_greedy), top_k 15 sampling
(k_sample) and K = 4 beams (k_beam_select).  "on" sets every processor: no_repeat_ngram_size 3, min_length, min_new_tokens 8, an EOS
decay, suppress and begin-suppress tokens, and min_p 0.05 on the sampled calls."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_beam import build_gpt          # noqa: E402
from genvc_amd import synth               # noqa: E402

PROC = dict(no_repeat_ngram_size=3, min_length=60, min_new_tokens=8, exponential_decay_length_penalty=(30, 1.05),
            suppress_tokens=[3, 700], begin_suppress_tokens=[5])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proc", choices=["on", "off"], required=True)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    g, dims = build_gpt()
    g.max_gen_mel_tokens = 40
    cond = synth.uniform(300, "cond_latents", (1, 32, dims["d_model"]), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    kw = PROC if args.proc == "on" else {}
    for _ in range(args.reps):
        g.generate(cond, codes, top_k=1, repetition_penalty=2.0, **kw)
        g.generate(cond, codes, top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0, seed=3,
                   **(dict(kw, min_p=0.05) if kw else {}))
        g.generate(cond, codes, num_beams=4, do_sample=False, repetition_penalty=2.0, beam_length_mode="generated", **kw)
    torch.cuda.synchronize()
    print("done", args.proc)


if __name__ == "__main__":
    main()
