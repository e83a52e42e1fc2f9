"""Cost of classifier-free guidance on one MI355X: full size (GenVC_small dims, synthetic weights, fp32), B items of
a 48-row prompt (32 conditioning latents + 13 content codes + 3), 200 greedy steps in ONE engine call, B in {1, 4, 8}.

    python scripts/bench_cfg.py [--out profiles/cfg_time.json] [--rounds 2] [--reps 5] [--parent-lib PATH/libgenvc_hip.so]

Two sides, each in a fresh child process (a process loads one library), alternating round by round:
  guided     engine.generate_cfg over B items = 2B rows: [guide, sample B rows, mirror, decode step over 2B rows] per step
  unguided   engine.generate over 2B rows: [sample 2B rows, decode step over 2B rows] per step -- the same decode work without guide and
             mirror.  With --parent-lib the child loads the PARENT commit's library (GENVC_HIP_LIB), so the comparator is the parent's
             own call; without it, this build's unguided call (the same code path: guidance off changes nothing).
Per side and B: device events around the call, which ends in a synchronise; the slots are prefilled again (untimed) before every
timed call, after one untimed call from the warmed graphs.  Reported per B: the median us per step of each side over all rounds and
reps, their ratio and difference, and `spread`, the largest relative distance of one timed call from its side's median: a difference
below it is not one.  The stop token is biased away so every run takes all its steps."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STEPS = 200
BS = (1, 4, 8)
CFG_SYMBOLS = ("gvc_cfg_guide", "gvc_gpt_generate_cfg", "gvc_gpt_warmup_cfg")


def med(xs):
    return sorted(xs)[len(xs) // 2]


def child(side, reps):
    import torch
    from genvc_amd import _lib
    if side == "unguided":
        for s in CFG_SYMBOLS:               # (the parent's library does not export them; this side never calls them)
            _lib._SIGNATURES.pop(s, None)
    from genvc_amd import synth
    from genvc_amd.engine import sample_params
    from time_contrastive import build_gpt
    g, dims = build_gpt(max_slots=16)
    eng = g.engine
    d = dims["d_model"]
    params = sample_params(dict(repetition_penalty=2.0, temperature=1.0, top_p=1.0, top_k=1), 1026, 1025)
    out = {}
    for B in BS:
        R = 2 * B
        cond = synth.uniform(300, "cond_latents", (R, 32, d), 1.0).cuda()
        codes = synth.integers(300, "content_codes", (R, 13), 256).cuda()
        prefix = eng.prefix_embeddings(cond, codes.int())
        n0 = int(prefix.shape[1]) + 1
        assert n0 == 48
        rows = B if side == "guided" else R
        slots = torch.arange(R, device="cuda", dtype=torch.int32)
        if side == "guided":
            eng.warmup_cfg(B, n0 + STEPS, 1)
        else:
            eng.warmup(R, n0 + STEPS, 1)
        toks = torch.zeros(rows, STEPS, device="cuda", dtype=torch.int32)
        lats = torch.zeros(rows, STEPS, d, device="cuda")

        def run(timed):
            eng.prefill(slots, prefix, want_outputs=False)
            ids = torch.ones(rows, n0 + STEPS + 8, device="cuda", dtype=torch.int32)
            ids[:, n0 - 1] = 1024
            ids_len = torch.full((rows,), n0, device="cuda", dtype=torch.int32)
            fin = torch.zeros(rows, device="cuda", dtype=torch.int32)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if side == "guided":
                eng.generate_cfg(slots[:B], slots[B:], 1.5, ids, ids_len, fin, params, None, 0, STEPS, toks, lats, max_keys=n0 + STEPS)
            else:
                eng.generate(slots, ids, ids_len, fin, params, 0, STEPS, toks, lats, max_keys=n0 + STEPS)
            e1.record()
            torch.cuda.synchronize()
            eng.health()
            return e0.elapsed_time(e1) * 1000.0 / STEPS
        run(False)
        base = eng.lazy_inits()
        out[str(B)] = dict(us_per_step=[run(True) for _ in range(reps)], variant=eng.decode_variant())
        assert eng.lazy_inits() == base, "a timed call allocated or captured"
    print("BENCH_CFG " + json.dumps(dict(side=side, device=torch.cuda.get_device_name(0), rows=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cfg_time.json"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--side", default=None, choices=["guided", "unguided"])
    args = ap.parse_args()
    if args.side:
        return child(args.side, args.reps)
    runs = {"guided": [], "unguided": []}
    device = None
    for _ in range(args.rounds):
        for side in ("guided", "unguided"):
            env = dict(os.environ)
            if side == "unguided" and args.parent_lib:
                env["GENVC_HIP_LIB"] = os.path.abspath(args.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--reps", str(args.reps)], env=env,
                               capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"{side} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("BENCH_CFG ")][-1]
            res = json.loads(line[len("BENCH_CFG "):])
            device = res["device"]
            runs[side].append(res["rows"])
    res = dict(device=device, steps=STEPS, n0=48, rounds=args.rounds, reps=args.reps,
               comparator="parent commit's library" if args.parent_lib else "this build's unguided call", rows={})
    for B in BS:
        gs = [x for r in runs["guided"] for x in r[str(B)]["us_per_step"]]
        us = [x for r in runs["unguided"] for x in r[str(B)]["us_per_step"]]
        mg, mu = med(gs), med(us)
        spread = max(max(abs(x - mg) / mg for x in gs), max(abs(x - mu) / mu for x in us))
        res["rows"][str(B)] = dict(items=B, decode_rows=2 * B, guided_us_per_step=mg, unguided_us_per_step=mu, ratio=mg / mu,
                                   added_us_per_step=mg - mu, spread=spread, guided_runs=gs, unguided_runs=us,
                                   variant=runs["guided"][0][str(B)]["variant"])
        print(f"B={B}: guided {mg:.1f} us/step, unguided over {2 * B} rows {mu:.1f} us/step, ratio {mg / mu:.4f}, "
              f"added {mg - mu:+.1f} us/step, spread {spread:.3%}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
