"""Per-launch cost of k_sample with the typical / epsilon / eta warpers off and on.

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python scripts/time_warpers.py --out <dir>/order.json
    python scripts/time_warpers.py --parse <dir>

The first form launches the sampler through gvc_sample / gvc_sample_warp on fixed random logits (vocab 1026, a 40-id history per row),
`--reps` launches per configuration, for B = 1 and 8 rows, top_k 0 / 15 / 50 (top_p 0.95, temperature 0.85, repetition penalty 2) and
the warpers off (gvc_sample: no warper pointer), each alone, and all three together; it writes the launch order.  The second form reads
the kernel trace, attributes the k_sample launches to their configurations in that order (one stream: they run in issue order) and
prints avg / median / min us per launch."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARPS = [("off", None), ("typical 0.5", dict(typical_p=0.5)), ("epsilon 3e-4", dict(epsilon_cutoff=3e-4)),
         ("eta 2e-3", dict(eta_cutoff=2e-3)), ("all three", dict(typical_p=0.5, epsilon_cutoff=3e-4, eta_cutoff=2e-3))]


def configs():
    """(B, top_k, name, warper kwargs) in launch order, a warm-up block first"""
    return [(8, 15, "warmup", dict(typical_p=0.5))] + [(B, k, name, kw) for B in (1, 8) for k in (0, 15, 50) for name, kw in WARPS]


def plan(reps):
    return [dict(B=B, top_k=k, warpers=name, n=reps) for B, k, name, _ in configs()]


def run(reps, out):
    import torch
    from genvc_amd import config as gcfg
    from genvc_amd.engine import GptEngine, logits_sets, sample_params
    V, EOS, n0 = 1026, 1025, 40
    eng = GptEngine(gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS), max_slots=8)
    gen = torch.Generator().manual_seed(4)
    for B, k, name, kw in configs():
        params = sample_params(dict(repetition_penalty=2.0, temperature=0.85, top_p=0.95, top_k=k), V, EOS, seed=1)
        logits = (torch.randn(B, V, generator=gen) * 2.0).cuda()
        ids = torch.randint(0, 1024, (B, n0 + 2), generator=gen).int().cuda()
        sets = logits_sets([kw] * B, n0, V) if kw else None
        for step in range(reps):
            ids_len = torch.full((B,), n0, device="cuda", dtype=torch.int32)
            fin = torch.zeros(B, device="cuda", dtype=torch.int32)
            if sets is None:
                eng.sample(logits, ids, ids_len, fin, params, step)
            else:
                eng.sample_warp(logits, ids, ids_len, fin, params, sets, step)
    torch.cuda.synchronize()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(plan(reps), f)
    print("done", len(configs()), "blocks")


def parse(d):
    order = json.load(open(os.path.join(d, "order.json")))
    path = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = []
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "k_sample" in name and "k_sample_greedy" not in name:
            rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0))
    rows.sort()
    assert len(rows) == sum(o["n"] for o in order), (len(rows), sum(o["n"] for o in order))
    print(f"{'B':>2} {'top_k':>5}  {'warpers':<13} {'n':>4} {'avg us':>8} {'median':>8} {'min us':>8}")
    i = 0
    for o in order:
        us = [t for _, t in rows[i:i + o["n"]]]
        i += o["n"]
        if o["warpers"] == "warmup":
            continue
        print(f"{o['B']:>2} {o['top_k']:>5}  {o['warpers']:<13} {len(us):>4} {statistics.mean(us):8.2f} {statistics.median(us):8.2f} "
              f"{min(us):8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default="order.json")
    ap.add_argument("--parse", default=None, help="a rocprofv3 output directory holding order.json")
    a = ap.parse_args()
    if a.parse:
        parse(a.parse)
    else:
        run(a.reps, a.out)


if __name__ == "__main__":
    main()
