"""Cost of the presence / frequency / windowed repetition penalties on the sampler of one MI355X: microseconds per
sampler call at B = 1 and B = 8 for top_k 1 / 15 / 0 over histories of 24 and 600 generated ids, on fixed logits of the model's
vocabulary (1026), medians of alternating rounds in ONE process.

    python scripts/time_penalties.py [--out profiles/penalties_time.json] [--rounds 7] [--calls 300]

Sides, interleaved call group by call group inside every round:
  plain     gvc_sample, no staging: the argmax kernel (k_sample_greedy) at top_k 1, k_sample otherwise
  off       gvc_sample_pen with a table whose one entry has everything off: the kernel of `plain` on the path every call without
            penalties takes -- no histogram -- behind the staging launches of the sides below, so the differences are the kernel's
  on        presence 0.5, frequency 0.25, no window: the histogram over the whole history and the penalties in the score loop
  windowed  the same with penalty_window 16 (the repetition penalty follows the counts)
  on_full   top_k 1 only: `on` beside a RAS table whose window is 0, which routes the call to the full kernel (k_sample) -- the
            alternative to giving the argmax kernel the histogram
A timed group is `calls` sampler calls between two device events, after one untimed group; every call resets the rows' lengths with one
tiny copy (the same on every side).  The sampler entries stage their tables per call, which costs the host more than the kernel runs at
top_k 1: there the groups measure the enqueue.  So the cost is ALSO measured where it is paid, in the captured generation loop at full
size (GenVC_small dims, synthetic weights, fp32, B = 1, a 48-row prompt, 200 steps in ONE engine call, the one-stream decode step),
microseconds per step, the sides alternating, the slot prefilled again (untimed) before every timed call:
  greedy / sample      gvc_gpt_generate at top_k 1 / 15: what the streaming path runs without the kwargs
  greedy_pen / sample_pen   gvc_gpt_generate_pen with presence 0.5, frequency 0.25, window 16 at the same top_k
  greedy_pen_full      the same at top_k 1 beside a RAS table that never redraws (min_count 65 of 64): the full kernel"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, EOS, P = 1026, 1025, 8
PEN = dict(presence_penalty=0.5, frequency_penalty=0.25)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def time_loop(rounds, steps=200):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from genvc_amd import synth
    from genvc_amd.engine import PenaltyTable, RasTable, logits_penalties, logits_ras, sample_params
    from time_contrastive import build_gpt
    g, dims = build_gpt(max_slots=8)
    eng = g.engine
    d = dims["d_model"]
    params = {k: sample_params(dict(repetition_penalty=1.0, temperature=0.85, top_p=0.85, top_k=k), V, EOS, seed=3) for k in (1, 15)}
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    prefix = eng.prefix_embeddings(cond, codes.int())
    n0 = int(prefix.shape[1]) + 1
    slots = torch.arange(1, device="cuda", dtype=torch.int32)
    for k in (1, 15):
        eng.warmup(1, n0 + steps, k)
    sides = ("greedy", "greedy_pen", "greedy_pen_full", "sample", "sample_pen")
    toks = {s: torch.zeros(1, steps, device="cuda", dtype=torch.int32) for s in sides}
    lats = torch.zeros(1, steps, d, device="cuda")
    pen = PenaltyTable([logits_penalties(dict(PEN, penalty_window=16), n0)])
    never = logits_ras(dict(ras_window=64), n0)
    never.min_count = 65
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ras = RasTable([never], cnt)

    def run(side):
        eng.prefill(slots, prefix, want_outputs=False)
        ids = torch.ones(1, n0 + steps + 8, device="cuda", dtype=torch.int32)
        ids[:, n0 - 1] = 1024
        ids_len = torch.full((1,), n0, device="cuda", dtype=torch.int32)
        fin = torch.zeros(1, device="cuda", dtype=torch.int32)
        p = params[1 if side.startswith("greedy") else 15]
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if side in ("greedy", "sample"):
            eng.generate(slots, ids, ids_len, fin, p, 0, steps, toks[side], lats, max_keys=n0 + steps)
        else:
            eng.generate_pen(slots, None, 1.0, ids, ids_len, fin, p, None, None, ras if side.endswith("_full") else None, pen, 0, steps,
                             toks[side], lats, max_keys=n0 + steps)
        e1.record()
        torch.cuda.synchronize()
        eng.health()
        return e0.elapsed_time(e1) * 1000.0 / steps
    for s in sides:
        run(s)
    base = eng.lazy_inits()
    times = {s: [] for s in sides}
    for _ in range(rounds):
        for s in sides:
            times[s].append(run(s))
    assert eng.lazy_inits() == base, "a timed call allocated or captured"
    assert torch.equal(toks["greedy_pen"], toks["greedy_pen_full"]) and int(cnt.sum()) == 0      # the two kernels: the same tokens
    u = {s: round(med(times[s]), 2) for s in sides}
    return dict(steps=steps, n0=n0, rounds=rounds, variant=eng.decode_variant(), us_per_step=u,
                us_per_step_min_max={s: [round(min(times[s]), 2), round(max(times[s]), 2)] for s in sides},
                greedy_pen_minus_greedy_us=round(u["greedy_pen"] - u["greedy"], 2),
                greedy_pen_full_minus_greedy_pen_us=round(u["greedy_pen_full"] - u["greedy_pen"], 2),
                sample_pen_minus_sample_us=round(u["sample_pen"] - u["sample"], 2),
                penalties_move_tokens=dict(greedy=not torch.equal(toks["greedy"], toks["greedy_pen"]),
                                           sample=not torch.equal(toks["sample"], toks["sample_pen"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "penalties_time.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--bench", default=None, help="a JSON file of bench.py headline results to record beside the timings")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_penalties.py measures on the GPU: none found")
    from genvc_amd import config as gcfg
    from genvc_amd import synth
    from genvc_amd.engine import GptEngine, PenaltyTable, RasTable, logits_penalties, sample_params
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    base = synth.uniform(4400, "penalties_time", (1, V), 3.0)[0]
    base[EOS] = -30.0
    results = []
    for B in (1, 8):
        logits = base[None].expand(B, V).contiguous().cuda()
        fin = torch.zeros(B, dtype=torch.int32, device="cuda")
        for H in (24, 600):
            ids = torch.ones(B, P + H + 8, dtype=torch.int32)
            ids[:, P:P + H] = synth.integers(4400 + H, "history", (B, H), 1024).int()
            ids = ids.cuda()
            len0 = torch.full((B,), P + H, dtype=torch.int32, device="cuda")
            ids_len = len0.clone()
            for top_k in (1, 15, 0):
                params = sample_params(dict(repetition_penalty=1.0, temperature=0.85, top_p=1.0, top_k=top_k), V, EOS, seed=7)
                tables = {"off": PenaltyTable([None]), "on": PenaltyTable([logits_penalties(PEN, P)]),
                          "windowed": PenaltyTable([logits_penalties(dict(PEN, penalty_window=16), P)])}
                sides = ("plain", "off", "on", "windowed") + (("on_full",) if top_k == 1 else ())
                to_full = RasTable([None])                  # (window 0: no RAS, but the call runs on k_sample)

                def group(side, step0):
                    for i in range(args.calls):
                        ids_len.copy_(len0)
                        if side == "plain":
                            eng.sample(logits, ids, ids_len, fin, params, step0 + i)
                        elif side == "on_full":
                            eng.sample_pen(logits, ids, ids_len, fin, params, tables["on"], step0 + i, ras=to_full)
                        else:
                            eng.sample_pen(logits, ids, ids_len, fin, params, tables[side], step0 + i)

                times = {s: [] for s in sides}
                for s in sides:
                    group(s, 0)                               # untimed: code objects, the allocator's pool
                torch.cuda.synchronize()
                for r in range(args.rounds):
                    for s in sides:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        group(s, 1000 * (r + 1))
                        e1.record()
                        torch.cuda.synchronize()
                        times[s].append(e0.elapsed_time(e1) * 1000.0 / args.calls)
                row = dict(B=B, history=H, top_k=top_k, calls_per_group=args.calls, rounds=args.rounds,
                           us_per_call={s: round(med(times[s]), 2) for s in sides},
                           us_per_call_min_max={s: [round(min(times[s]), 2), round(max(times[s]), 2)] for s in sides})
                u = row["us_per_call"]
                row["on_minus_off_us"] = round(u["on"] - u["off"], 2)
                row["windowed_minus_off_us"] = round(u["windowed"] - u["off"], 2)
                row["off_minus_plain_us"] = round(u["off"] - u["plain"], 2)          # the staging launches
                if top_k == 1:
                    row["on_full_minus_on_us"] = round(u["on_full"] - u["on"], 2)    # the full kernel (and one more staging launch)
                results.append(row)
                print(json.dumps(row))
    eng.close()
    loop = time_loop(args.rounds)
    print(json.dumps(loop))
    out = dict(device=torch.cuda.get_device_name(0), vocab=V, penalties=PEN, results=results, generation_loop=loop)
    if args.bench:
        with open(args.bench) as f:
            out["bench"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
