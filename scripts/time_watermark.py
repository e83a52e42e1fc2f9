"""Cost of the green-list watermark on the sampler of one MI355X, and of its detector: medians of alternating rounds
in ONE process.

    python scripts/time_watermark.py [--out profiles/watermark_time.json] [--rounds 7] [--calls 300]

Per sampler call at B = 1 and B = 8 for top_k 1 (greedy) / 15 / 0, on fixed logits of the model's vocabulary (1026), the sides
interleaved call group by call group inside every round:
  plain     gvc_sample, no staging: the argmax kernel (k_sample_greedy) at top_k 1, k_sample otherwise
  off       gvc_sample_wm with an entry whose table is null: the kernel of `plain` behind the staging launches of the sides below
  lefthash  the table row of the previous id staged in LDS, the bias on the green survivors, one more workgroup maximum
  selfhash  the one-row table and the 40-highest-scores condition
  left_full top_k 1 only: `lefthash` beside a RAS table whose window is 0, which routes the call to the full kernel (k_sample) -- the
            alternative to giving the argmax kernel the table
The sampler entries stage their entries per call, which costs the host more than the kernel runs at top_k 1: there the groups measure
the enqueue.  So the cost is ALSO measured where it is paid, in the captured generation loop at full size (GenVC_small dims, synthetic
weights, fp32, B = 1, a 48-row prompt, 200 steps in ONE engine call, the one-stream decode step), microseconds per step, the slot
prefilled again (untimed) before every timed call:
  greedy / sample          gvc_gpt_generate at top_k 1 / 15
  greedy_wm / sample_wm    gvc_gpt_generate_wm with a lefthash table at the same top_k
  greedy_wm_full           the same at top_k 1 beside a RAS table that never redraws: the full kernel
The detector: microseconds per gvc_wm_score call at B = 8, n = 600, lefthash, with and without ignore_repeated_ngrams."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, EOS, P = 1026, 1025, 8
CFG = dict(greenlist_ratio=0.25, bias=2.0, hashing_key=15485863, seeding_scheme="lefthash", context_width=1)


def med(xs):
    return sorted(xs)[len(xs) // 2]


def time_loop(rounds, steps=200):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from genvc_amd import synth
    from genvc_amd.engine import RasTable, WatermarkTable, logits_ras, sample_params, watermark_settings
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
    sides = ("greedy", "greedy_wm", "greedy_wm_full", "sample", "sample_wm")
    toks = {s: torch.zeros(1, steps, device="cuda", dtype=torch.int32) for s in sides}
    lats = torch.zeros(1, steps, d, device="cuda")
    wm = WatermarkTable([eng.watermark_entry(watermark_settings(dict(watermarking_config=CFG), V))], eng)
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
            eng.generate_wm(slots, None, 1.0, ids, ids_len, fin, p, None, None, ras if side.endswith("_full") else None, None, wm, 0,
                            steps, toks[side], lats, max_keys=n0 + steps)
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
    assert eng.lazy_inits() == base and eng.watermark_uploads() == 1, "a timed call allocated, uploaded or captured"
    assert torch.equal(toks["greedy_wm"], toks["greedy_wm_full"]) and int(cnt.sum()) == 0      # the two kernels: the same tokens
    u = {s: round(med(times[s]), 2) for s in sides}
    return dict(steps=steps, n0=n0, rounds=rounds, variant=eng.decode_variant(), us_per_step=u,
                us_per_step_min_max={s: [round(min(times[s]), 2), round(max(times[s]), 2)] for s in sides},
                greedy_wm_minus_greedy_us=round(u["greedy_wm"] - u["greedy"], 2),
                greedy_wm_full_minus_greedy_wm_us=round(u["greedy_wm_full"] - u["greedy_wm"], 2),
                sample_wm_minus_sample_us=round(u["sample_wm"] - u["sample"], 2),
                mark_moves_tokens=dict(greedy=not torch.equal(toks["greedy"], toks["greedy_wm"]),
                                       sample=not torch.equal(toks["sample"], toks["sample_wm"])))


def time_detector(rounds, calls):
    import torch
    from genvc_amd.engine import WatermarkDetector
    codes = torch.randint(0, 1024, (8, 600), generator=torch.Generator().manual_seed(3)).cuda()
    out = {}
    for ignore in (False, True):
        det = WatermarkDetector(CFG, V, ignore_repeated_ngrams=ignore)
        for _ in range(20):
            det.counts(codes)
        torch.cuda.synchronize()
        ts = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                det.counts(codes)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1000.0 / calls)
        out["ignore_repeated" if ignore else "plain"] = dict(us_per_call=round(med(ts), 2), min_max=[round(min(ts), 2), round(max(ts), 2)])
    return dict(B=8, n=600, scheme="lefthash", calls_per_group=calls, rounds=rounds, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "watermark_time.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--bench", default=None, help="a JSON file of bench.py headline results to record beside the timings")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_watermark.py measures on the GPU: none found")
    from genvc_amd import config as gcfg
    from genvc_amd import synth
    from genvc_amd.engine import GptEngine, RasTable, WatermarkTable, sample_params, watermark_settings
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=4)
    base = synth.uniform(4400, "watermark_time", (1, V), 3.0)[0]
    base[EOS] = -30.0
    tables = {"off": WatermarkTable([None])}
    for scheme in ("lefthash", "selfhash"):
        s = watermark_settings(dict(watermarking_config=dict(CFG, seeding_scheme=scheme)), V)
        tables[scheme] = WatermarkTable([eng.watermark_entry(s)], eng)
    results = []
    H = 24
    for B in (1, 8):
        logits = base[None].expand(B, V).contiguous().cuda()
        fin = torch.zeros(B, dtype=torch.int32, device="cuda")
        ids = torch.ones(B, P + H + 8, dtype=torch.int32)
        ids[:, P:P + H] = synth.integers(4400 + H, "history", (B, H), 1024).int()
        ids = ids.cuda()
        len0 = torch.full((B,), P + H, dtype=torch.int32, device="cuda")
        ids_len = len0.clone()
        for top_k in (1, 15, 0):
            params = sample_params(dict(repetition_penalty=1.0, temperature=0.85, top_p=1.0, top_k=top_k), V, EOS, seed=7)
            sides = ("plain", "off", "lefthash", "selfhash") + (("left_full",) if top_k == 1 else ())
            to_full = RasTable([None])                  # (window 0: no RAS, but the call runs on k_sample)

            def group(side, step0):
                for i in range(args.calls):
                    ids_len.copy_(len0)
                    if side == "plain":
                        eng.sample(logits, ids, ids_len, fin, params, step0 + i)
                    elif side == "left_full":
                        eng.sample_wm(logits, ids, ids_len, fin, params, tables["lefthash"], step0 + i, ras=to_full)
                    else:
                        eng.sample_wm(logits, ids, ids_len, fin, params, tables[side], step0 + i)

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
            row["lefthash_minus_off_us"] = round(u["lefthash"] - u["off"], 2)
            row["selfhash_minus_off_us"] = round(u["selfhash"] - u["off"], 2)
            row["off_minus_plain_us"] = round(u["off"] - u["plain"], 2)          # the staging launches
            if top_k == 1:
                row["left_full_minus_lefthash_us"] = round(u["left_full"] - u["lefthash"], 2)
            results.append(row)
            print(json.dumps(row))
    for t in tables.values():
        t.release()
    eng.close()
    det = time_detector(args.rounds, args.calls)
    print(json.dumps(det))
    loop = time_loop(args.rounds)
    print(json.dumps(loop))
    out = dict(device=torch.cuda.get_device_name(0), vocab=V, watermarking_config=CFG, results=results, detector=det, generation_loop=loop)
    if args.bench:
        with open(args.bench) as f:
            out["bench"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
