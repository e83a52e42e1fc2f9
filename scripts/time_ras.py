"""Cost of repetition-aware sampling on the sampler of one MI355X: microseconds per sampler call at B = 1 and B = 8 for
top_k 1 / 15 / 50 on fixed logits of the model's vocabulary (1026), medians of alternating rounds in ONE process.

    python scripts/time_ras.py [--out profiles/ras_time.json] [--rounds 7] [--calls 300]

Sides, interleaved call group by call group inside every round:
  off      gvc_sample_ras with a table whose window is 0: the full kernel (k_sample) on the path every call without RAS takes -- no count,
           no extra barrier -- behind the same staging launches as the two sides below, so the differences are the kernel's
  count    RAS on (window 64, min_count 1) over a history of 64 distinct ids none of which can be drawn: the count and its one
           reduction run at every step, nothing is drawn again (the redraw counters stay 0: asserted)
  redraw   RAS on over a history that holds every id the truncated set can draw: every step draws again (the counters equal the calls:
           asserted)
  plain    gvc_sample, no staging: k_sample for top_k 15 / 50, the argmax kernel (k_sample_greedy) for top_k 1 -- what a call without
           RAS costs, and for top_k 1 the price of the escape hatch: `off`/`count` at top_k 1 against it
A timed group is `calls` sampler calls between two device events, after one untimed group; every call resets the rows' lengths with one
tiny copy (the same on every side).  Repetition penalty 1: the histories do not move the scores.

The sampler entries stage their tables per call, which at top_k 1 costs the host more than the kernel runs: there the groups measure the
enqueue, not the kernel.  So the price of the escape hatch is ALSO measured where it is paid, in the captured generation loop at full size
(GenVC_small dims, synthetic weights, fp32, B = 1, a 48-row prompt, 200 steps in ONE engine call, the one-stream decode step),
microseconds per step, the sides alternating, the slot prefilled again (untimed) before every timed call:
  greedy   gvc_gpt_generate at top_k 1: the argmax kernel (k_sample_greedy), what the streaming path runs today
  count    gvc_gpt_generate_ras at top_k 1 with a count no window can reach (min_count 65 of 64, hand-set): the full kernel counts at
           every step and never draws again; its tokens are the greedy ones (asserted)
  redraw   the same with min_count 1: it draws again whenever the argmax is among the row's last 64 tokens (the counter is reported)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, EOS, P, K = 1026, 1025, 8, 64
SIDES = ("plain", "off", "count", "redraw")


def med(xs):
    return sorted(xs)[len(xs) // 2]


def time_loop(rounds, steps=200):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from genvc_amd import synth
    from genvc_amd.engine import RasTable, logits_ras, sample_params
    from time_contrastive import build_gpt
    g, dims = build_gpt(max_slots=8)
    eng = g.engine
    d = dims["d_model"]
    params = sample_params(dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=1), V, EOS, seed=3)
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    prefix = eng.prefix_embeddings(cond, codes.int())
    n0 = int(prefix.shape[1]) + 1
    slots = torch.arange(1, device="cuda", dtype=torch.int32)
    for k in (1, 0):
        eng.warmup(1, n0 + steps, k)
    toks = {s: torch.zeros(1, steps, device="cuda", dtype=torch.int32) for s in ("greedy", "count", "redraw")}
    lats = torch.zeros(1, steps, d, device="cuda")
    cnt = {s: torch.zeros(1, dtype=torch.int32, device="cuda") for s in ("count", "redraw")}
    never = logits_ras(dict(ras_window=K), n0)
    never.min_count = K + 1
    always = logits_ras(dict(ras_window=K, ras_threshold=1.0 / K), n0)
    tables = {"count": RasTable([never], cnt["count"]), "redraw": RasTable([always], cnt["redraw"])}

    def run(side):
        eng.prefill(slots, prefix, want_outputs=False)
        ids = torch.ones(1, n0 + steps + 8, device="cuda", dtype=torch.int32)
        ids[:, n0 - 1] = 1024
        ids_len = torch.full((1,), n0, device="cuda", dtype=torch.int32)
        fin = torch.zeros(1, device="cuda", dtype=torch.int32)
        if side != "greedy":
            cnt[side].zero_()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if side == "greedy":
            eng.generate(slots, ids, ids_len, fin, params, 0, steps, toks[side], lats, max_keys=n0 + steps)
        else:
            eng.generate_ras(slots, None, 1.0, ids, ids_len, fin, params, None, None, tables[side], 0, steps, toks[side], lats,
                             max_keys=n0 + steps)
        e1.record()
        torch.cuda.synchronize()
        eng.health()
        return e0.elapsed_time(e1) * 1000.0 / steps
    sides = ("greedy", "count", "redraw")
    for s in sides:
        run(s)
    base = eng.lazy_inits()
    times = {s: [] for s in sides}
    for _ in range(rounds):
        for s in sides:
            times[s].append(run(s))
    assert eng.lazy_inits() == base, "a timed call allocated or captured"
    assert torch.equal(toks["greedy"], toks["count"]) and int(cnt["count"].sum()) == 0
    u = {s: round(med(times[s]), 2) for s in sides}
    return dict(steps=steps, n0=n0, rounds=rounds, variant=eng.decode_variant(), us_per_step=u,
                us_per_step_min_max={s: [round(min(times[s]), 2), round(max(times[s]), 2)] for s in sides},
                count_minus_greedy_us=round(u["count"] - u["greedy"], 2), redraw_minus_count_us=round(u["redraw"] - u["count"], 2),
                redraws_of_steps=[int(cnt["redraw"].sum()), steps])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ras_time.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_ras.py measures on the GPU: none found")
    from genvc_amd import config as gcfg
    from genvc_amd import synth
    from genvc_amd.engine import GptEngine, RasTable, logits_ras, sample_params
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    base = synth.uniform(4300, "ras_time", (1, V), 3.0)[0]
    base[EOS] = -30.0
    order = torch.argsort(base, descending=True)
    top = [int(t) for t in order[:50]]                    # every id a top_k <= 50 call can draw
    cold = [int(t) for t in order[-K:]]                   # 64 distinct ids ...
    base[cold] = -30.0                                    # ... that no call draws
    results = []
    for B in (1, 8):
        logits = base[None].expand(B, V).contiguous().cuda()
        fin = torch.zeros(B, dtype=torch.int32, device="cuda")
        hist = {"count": cold, "redraw": (top + cold)[:K], "off": cold, "plain": cold}
        ids, len0 = {}, torch.full((B,), P + K, dtype=torch.int32, device="cuda")
        for side, h in hist.items():
            t = torch.ones(B, P + K + 8, dtype=torch.int32)
            t[:, P:P + K] = torch.tensor(h, dtype=torch.int32)
            ids[side] = t.cuda()
        ids_len = len0.clone()
        for top_k in (1, 15, 50):
            params = sample_params(dict(repetition_penalty=1.0, temperature=0.85, top_p=1.0, top_k=top_k), V, EOS, seed=7)
            cnt = {s: torch.zeros(B, dtype=torch.int32, device="cuda") for s in SIDES}
            on = logits_ras(dict(ras_window=K, ras_threshold=1.0 / K), P)
            assert (on.window, on.min_count) == (K, 1)
            tables = {"off": RasTable([None], cnt["off"]), "count": RasTable([on], cnt["count"]), "redraw": RasTable([on], cnt["redraw"])}

            def group(side, step0):
                for i in range(args.calls):
                    ids_len.copy_(len0)
                    if side == "plain":
                        eng.sample(logits, ids[side], ids_len, fin, params, step0 + i)
                    else:
                        eng.sample_ras(logits, ids[side], ids_len, fin, params, tables[side], step0 + i)

            times = {s: [] for s in SIDES}
            for s in SIDES:
                group(s, 0)                               # untimed: code objects, the allocator's pool
            torch.cuda.synchronize()
            for c in cnt.values():
                c.zero_()
            for r in range(args.rounds):
                for s in SIDES:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    group(s, 1000 * (r + 1))
                    e1.record()
                    torch.cuda.synchronize()
                    times[s].append(e0.elapsed_time(e1) * 1000.0 / args.calls)
            n = args.rounds * args.calls
            assert int(cnt["off"].sum()) == 0 and int(cnt["count"].sum()) == 0, "the no-redraw sides drew again"
            assert cnt["redraw"].cpu().tolist() == [n] * B, f"the redraw side drew again {cnt['redraw'].cpu().tolist()} times, not {n}"
            row = dict(B=B, top_k=top_k, calls_per_group=args.calls, rounds=args.rounds,
                       us_per_call={s: round(med(times[s]), 2) for s in SIDES},
                       us_per_call_min_max={s: [round(min(times[s]), 2), round(max(times[s]), 2)] for s in SIDES})

            u = row["us_per_call"]
            row["count_minus_off_us"] = round(u["count"] - u["off"], 2)
            row["redraw_minus_count_us"] = round(u["redraw"] - u["count"], 2)
            row["off_minus_plain_us"] = round(u["off"] - u["plain"], 2)          # staging launches (+ the full kernel at top_k 1)
            results.append(row)
            print(json.dumps(row))
    eng.close()
    loop = time_loop(args.rounds)
    print(json.dumps(loop))
    out = dict(device=torch.cuda.get_device_name(0), vocab=V, window=K, sides=list(SIDES), results=results, generation_loop=loop)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
