"""Cost of sequence_bias / bad_words_ids / forced_eos_token_id / renormalize_logits on one MI355X: full size (GenVC_small
dims, synthetic weights, fp32), B streams of a 48-row prompt (32 conditioning latents + 13 content codes + 3), 200 greedy steps in ONE
engine call, B in {1, 4, 8}.

    python scripts/bench_logits_bias.py --parent-lib PATH/libgenvc_hip.so [--out profiles/logits_bias_time.json] [--rounds 3] [--reps 5]

Three sides, each in a fresh child process (a process loads one library), interleaved round by round:
  parent   engine.generate on the PARENT commit's library (GENVC_HIP_LIB)
  off      engine.generate on this build: the kwargs off, the call every existing caller makes
  on       engine.generate_bias on this build with 32 entries (16 length-1 biases, which hit at every step, 8 longer ones and 8 bad
           words), the forced EOS and renormalised scores stored at every step
Per side and B: device events around the call, which ends in a synchronise; the slots are prefilled again (untimed) before every
timed call, after one untimed call from the warmed graphs.  Reported per B:
  (a) off against parent: the medians, their difference, and the bar -- the parent's own run-to-run spread in this session (the largest
      relative distance of one of its timed calls from its median); `within_bar` says whether the difference stays inside it
  (b) on against off: the medians and the added us per step; reported only, no bar.
The stop token is biased away so every run takes all its steps."""
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
NEW_SYMBOLS = ("gvc_sample_bias", "gvc_gpt_generate_bias")
SIDES = ("parent", "off", "on")


def med(xs):
    return sorted(xs)[len(xs) // 2]


def child(side, reps):
    import torch
    from genvc_amd import _lib
    if side == "parent":
        for s in NEW_SYMBOLS:               # (the parent's library does not export them; this side never calls them)
            _lib._SIGNATURES.pop(s, None)
    from genvc_amd import synth
    from genvc_amd.engine import logits_bias, sample_params
    from time_contrastive import build_gpt
    g, dims = build_gpt(max_slots=8)
    eng = g.engine
    d, V = dims["d_model"], dims["num_audio_tokens"]
    params = sample_params(dict(repetition_penalty=2.0, temperature=1.0, top_p=1.0, top_k=1), V, 1025)
    out = {}
    for B in BS:
        cond = synth.uniform(300, "cond_latents", (B, 32, d), 1.0).cuda()
        codes = synth.integers(300, "content_codes", (B, 13), 256).cuda()
        prefix = eng.prefix_embeddings(cond, codes.int())
        n0 = int(prefix.shape[1]) + 1
        assert n0 == 48
        slots = torch.arange(B, device="cuda", dtype=torch.int32)
        eng.warmup(B, n0 + STEPS, 1)
        toks = torch.zeros(B, STEPS, device="cuda", dtype=torch.int32)
        lats = torch.zeros(B, STEPS, d, device="cuda")
        scores = torch.zeros(B, STEPS, V, device="cuda") if side == "on" else None
        bias = None
        if side == "on":
            kw = dict(sequence_bias={**{(100 + i,): -0.25 for i in range(16)}, **{(200 + i, 300 + i, 400 + i): 1.0 for i in range(8)}},
                      bad_words_ids=[[500 + i, 600 + i] for i in range(8)], forced_eos_token_id=1025, renormalize_logits=True)
            bias = logits_bias(kw, n0, STEPS, V, 1025)
            assert bias.n_bias + bias.n_ban == 32

        def run():
            eng.prefill(slots, prefix, want_outputs=False)
            ids = torch.ones(B, n0 + STEPS + 8, device="cuda", dtype=torch.int32)
            ids[:, n0 - 1] = 1024
            ids_len = torch.full((B,), n0, device="cuda", dtype=torch.int32)
            fin = torch.zeros(B, device="cuda", dtype=torch.int32)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if side == "on":
                eng.generate_bias(slots, None, 1.0, ids, ids_len, fin, params, None, bias, 0, STEPS, toks, lats, scores_out=scores,
                                  do_sample=False, max_keys=n0 + STEPS)
            else:
                eng.generate(slots, ids, ids_len, fin, params, 0, STEPS, toks, lats, max_keys=n0 + STEPS)
            e1.record()
            torch.cuda.synchronize()
            eng.health()
            return e0.elapsed_time(e1) * 1000.0 / STEPS
        run()
        base = eng.lazy_inits()
        out[str(B)] = dict(us_per_step=[run() for _ in range(reps)], variant=eng.decode_variant(), tokens=toks.cpu().tolist())
        assert eng.lazy_inits() == base, "a timed call allocated or captured"
    print("BENCH_BIAS " + json.dumps(dict(side=side, device=torch.cuda.get_device_name(0), rows=out)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logits_bias_time.json"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--side", default=None, choices=SIDES)
    args = ap.parse_args()
    if args.side:
        return child(args.side, args.reps)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libgenvc_hip.so is the comparator of (a); build it from a checkout of the parent")
    runs = {s: [] for s in SIDES}
    device = None
    for rnd in range(args.rounds):
        for side in SIDES:
            print(f"round {rnd + 1} of {args.rounds}: {side}", flush=True)
            env = dict(os.environ)
            if side == "parent":
                env["GENVC_HIP_LIB"] = os.path.abspath(args.parent_lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--side", side, "--reps", str(args.reps)], env=env,
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"{side} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("BENCH_BIAS ")][-1]
            res = json.loads(line[len("BENCH_BIAS "):])
            device = res["device"]
            runs[side].append(res["rows"])
    res = dict(device=device, steps=STEPS, n0=48, rounds=args.rounds, reps=args.reps, rows={})
    for B in BS:
        t = {s: [x for r in runs[s] for x in r[str(B)]["us_per_step"]] for s in SIDES}
        m = {s: med(t[s]) for s in SIDES}
        spread = {s: max(abs(x - m[s]) / m[s] for x in t[s]) for s in SIDES}
        same = all(r[str(B)]["tokens"] == runs["parent"][0][str(B)]["tokens"] for s in ("parent", "off") for r in runs[s])
        forced = all(row[-1] == 1025 for r in runs["on"] for row in r[str(B)]["tokens"])
        res["rows"][str(B)] = dict(streams=B, variant=runs["off"][0][str(B)]["variant"], off_tokens_equal_parent=same, on_ends_in_eos=forced,
                                   parent_us_per_step=m["parent"], off_us_per_step=m["off"], on_us_per_step=m["on"],
                                   off_minus_parent_us=m["off"] - m["parent"], off_over_parent=m["off"] / m["parent"],
                                   bar_parent_spread=spread["parent"], within_bar=abs(m["off"] - m["parent"]) / m["parent"] <= spread["parent"],
                                   on_minus_off_us=m["on"] - m["off"], on_over_off=m["on"] / m["off"], spread=spread,
                                   parent_runs=t["parent"], off_runs=t["off"], on_runs=t["on"])
        print(f"B={B}: parent {m['parent']:.1f}, off {m['off']:.1f} ({m['off'] - m['parent']:+.2f} us/step, bar +-{spread['parent']:.3%} "
              f"= +-{spread['parent'] * m['parent']:.2f} us), on {m['on']:.1f} ({m['on'] - m['off']:+.2f} us/step over off); off tokens equal parent {same}, on ends in the stop token {forced}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
