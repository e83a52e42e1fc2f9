"""One-stream decode launches of a bench.py run from a rocprofv3 kernel trace, and what runs in front of each prefill:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py --gpus 1 --steps K --warmup W
    python scripts/deferred_decode_trace.py DIR/.../*_kernel_trace.csv <utterances = K + W>

k_decode_persist launches are split at 100 us into full steps and early exits (a launch that finds its run flag down: the first step of
a deferring call with nothing pending).  The second table lists the three kernels in front of every k_embed_rows dispatch (the first
launch of a prefill): with the eager order a chunk's last k_decode_persist sits there, feeding nobody but k_gen_end."""
import collections
import csv
import sys


def short(name):
    name = name.split("(")[0]
    for k in ("k_decode_persist", "k_gen_end_defer", "k_gen_end", "k_gen_begin", "k_sample_greedy", "k_sample", "k_embed_rows", "k_set_state",
              "k_stage_rows", "k_flush_begin"):
        if k in name:
            return k
    return name[:48]


rows = list(csv.DictReader(open(sys.argv[1])))
utt = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
names = [short(r["Kernel_Name"]) for r in rows]
dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]

full = [d for n, d in zip(names, dur) if n == "k_decode_persist" and d >= 100.0]
early = [d for n, d in zip(names, dur) if n == "k_decode_persist" and d < 100.0]
for tag, v in (("full steps", full), ("early exits", early)):
    if v:
        v = sorted(v)
        print(f"k_decode_persist {tag:11s}: n={len(v):5d} ({len(v) / utt:6.1f} per utterance)  avg {sum(v) / len(v):7.1f}  median {v[len(v) // 2]:7.1f}  "
              f"min {v[0]:7.1f}  max {v[-1]:7.1f} us")
    else:
        print(f"k_decode_persist {tag:11s}: none")
for k in ("k_gen_begin", "k_gen_end", "k_gen_end_defer", "k_sample_greedy", "k_flush_begin"):
    v = [d for n, d in zip(names, dur) if n == k]
    if v:
        print(f"{k:28s}: n={len(v):5d} ({len(v) / utt:6.1f} per utterance)  avg {sum(v) / len(v):7.1f} us")

tails = collections.Counter()
for i, n in enumerate(names):
    if n == "k_embed_rows" and i >= 3:
        tails[" -> ".join(names[i - 3:i])] += 1
print("kernels in front of a prefill's first launch (k_embed_rows):")
for t, c in tails.most_common(8):
    print(f"  {c:5d} x  {t}")
