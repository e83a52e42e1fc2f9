"""Cost of num_return_sequences = N on one MI355X: full size (GenVC_small dims, synthetic weights, fp32), one item, a
48-row prompt (32 conditioning latents + 13 content codes + 3), 24 steps, N in {1, 2, 4, 8}.

    python scripts/time_nbest.py [--out profiles/nbest_time.json] [--reps 9] [--ns 1 2 4 8] [--profile] [--comparators-only]

Per N (device events around work that ends in a synchronise; medians over `reps` runs, every run's figure kept):
  prefill_fanout_ms   one single-item prefill + the fan-out to the N - 1 other slots
  prefill_repeat_ms   comparator (b)'s prefill: one N-row prefill of the N-fold repeated prefix
  ms_per_step         the N-row sampled decode, 24 steps from the warmed graphs
  call_ms             GPT.generate(num_return_sequences=N), whole call (host work and the candidates' score included)
  successive_ms       comparator (a): N successive GPT.generate calls, seeds 0 .. N-1
  repeat_ms           comparator (b): one GPT.generate on repeat_interleave(N) inputs
  fanout_bytes, fanout_us, fanout_GBps   bytes the fan-out writes (the cache spans, as many read) over its own device time
The three whole calls are timed alternately inside one repetition (call, successive, repeat, call, ...), and `spread` is the largest
relative distance of a repetition's call_ms from the median: a difference below it is not one.  --comparators-only times (a), (b) and
(b)'s prefill alone, through calls the parent commit has too: run from a checkout of the parent (this file copied into its scripts/)
it gives the comparators' times there (`profiles/nbest_time_parent.json`).  `score_ms`: sequence_logprobs for [8, 240].  --profile: one untimed pass of every N for a
`rocprofv3 --kernel-trace --stats` run (no figures written).  The stop token is biased away so every run takes all its steps."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from genvc_amd import synth               # noqa: E402
from time_contrastive import build_gpt    # noqa: E402

STEPS = 24


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbest_time.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ns", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--comparators-only", action="store_true")
    args = ap.parse_args()
    g, dims = build_gpt(max_slots=8)
    eng = g.engine
    d, L, H = dims["d_model"], dims["n_layer"], dims["n_head"]
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    fake = g.compute_embeddings(cond, codes)
    prefix = g._prefix
    n0 = int(fake.shape[1])
    assert n0 == 48
    kw = dict(do_sample=True, top_k=15, top_p=0.85, temperature=0.75, repetition_penalty=2.0, max_new_tokens=STEPS, group=8)
    for N in sorted(set(args.ns) | {1}):
        eng.warmup_range(N, n0 + 8, n0 + STEPS, 15)
    res = dict(device=torch.cuda.get_device_name(0), n0=n0, steps=STEPS, reps=args.reps, rows={})
    for N in args.ns:
        slots = torch.arange(N, device="cuda", dtype=torch.int32)
        src, dst = slots[:1].repeat_interleave(max(N - 1, 1)), slots[1:].contiguous()
        rep_prefix = prefix.repeat_interleave(N, 0).contiguous()
        fakeN = fake.repeat_interleave(N, 0)
        condN, codesN = cond.repeat_interleave(N, 0), codes.repeat_interleave(N, 0)

        def prefill_fanout():
            eng.prefill(slots[:1], prefix, want_outputs=False)
            if N > 1:
                eng.kv_fanout(src, dst)

        def fanout():
            if N > 1:
                eng.kv_fanout(src, dst)

        def prefill_repeat():
            eng.prefill(slots, rep_prefix, want_outputs=False)

        def decode():
            g.compute_embeddings(cond, codes)                    # (the stored prefix: one row per item)
            st = g._start(fakeN, dict(kw), fan=N)
            torch.cuda.synchronize()
            return st

        def call():
            g.generate(cond, codes, num_return_sequences=N, seed=1, **kw)

        def successive():
            for j in range(N):
                g.generate(cond, codes, seed=j, **kw)

        def repeat():
            g.generate(condN, codesN, seed=1, **kw)

        if args.profile:
            call(), successive(), repeat()
            continue
        if args.comparators_only:
            for fn in (successive, repeat, prefill_repeat):
                fn()
            row = dict(successive_ms=[], repeat_ms=[], prefill_repeat_ms=[])
            for _ in range(args.reps):
                row["successive_ms"].append(timed(successive))
                row["repeat_ms"].append(timed(repeat))
                row["prefill_repeat_ms"].append(timed(prefill_repeat))
            out = {k: med(v) for k, v in row.items()}
            out.update(N=N, all=row, spread=max(abs(x - out["repeat_ms"]) for x in row["repeat_ms"]) / out["repeat_ms"])
            res["rows"][f"N{N}"] = out
            print(f"N={N}: successive {out['successive_ms']:.2f} ms, repeat {out['repeat_ms']:.2f} ms (spread {100 * out['spread']:.1f} %), "
                  f"N-row prefill {out['prefill_repeat_ms']:.3f} ms", flush=True)
            continue
        for fn in (call, successive, repeat, prefill_fanout, prefill_repeat):      # (first use of every shape is not timed)
            fn()
        row = dict(N=N, call_ms=[], successive_ms=[], repeat_ms=[], prefill_fanout_ms=[], prefill_repeat_ms=[], fanout_us=[],
                   step_ms=[])
        for _ in range(args.reps):
            row["call_ms"].append(timed(call))
            row["successive_ms"].append(timed(successive))
            row["repeat_ms"].append(timed(repeat))
            row["prefill_fanout_ms"].append(timed(prefill_fanout))
            row["prefill_repeat_ms"].append(timed(prefill_repeat))
            row["fanout_us"].append(1e3 * timed(fanout))
            st = decode()
            row["step_ms"].append(timed(lambda: g._advance(st, STEPS)) / STEPS)
        out = {k: med(v) for k, v in row.items() if isinstance(v, list)}
        out.update(N=N, all={k: v for k, v in row.items() if isinstance(v, list)},
                   spread=max(abs(x - out["call_ms"]) for x in row["call_ms"]) / out["call_ms"])
        out["ms_per_step"] = out.pop("step_ms")
        # the fan-out writes (N - 1) x [L][k|v][H][n0][hd] fp32 cache rows and reads as many (plus 3 x (V + d) floats of parked state)
        out["fanout_bytes"] = (N - 1) * 2 * L * H * n0 * (d // H) * 4
        out["fanout_GBps"] = 2 * out["fanout_bytes"] / (out["fanout_us"] * 1e-6) / 1e9 if N > 1 else 0.0
        res["rows"][f"N{N}"] = out
        print(f"N={N}: call {out['call_ms']:.2f} ms (spread {100 * out['spread']:.1f} %), successive {out['successive_ms']:.2f}, "
              f"repeat {out['repeat_ms']:.2f}; prefill+fanout {out['prefill_fanout_ms']:.3f} vs N-row prefill "
              f"{out['prefill_repeat_ms']:.3f} ms; {out['ms_per_step']:.3f} ms/step; fan-out {out['fanout_us']:.1f} us, "
              f"{out['fanout_GBps']:.0f} GB/s", flush=True)
    if args.comparators_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    if args.profile:
        g.sequence_logprobs(torch.zeros(8, 240, dtype=torch.long, device="cuda"), torch.zeros(8, 240, d, device="cuda"))
        torch.cuda.synchronize()
        return
    toks = torch.randint(0, 1024, (8, 240), device="cuda", dtype=torch.int32)
    lats = torch.randn(8, 240, d, device="cuda")
    eng.sequence_logprobs(toks, lats)
    ts = [timed(lambda: eng.sequence_logprobs(toks, lats)) for _ in range(args.reps)]
    res["score_ms"] = dict(shape=[8, 240], ms=med(ts), all=ts)
    print(f"sequence_logprobs [8, 240]: {med(ts):.3f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
