"""tests/golden/group_beam.npz: group (diverse) beam search -- GPT.generate(num_beams=K, num_beam_groups=G, diversity_penalty=lam,
do_sample=False, ...) -- computed by the CPU restatement tests/group_beam_oracle.py on the oracle's GPT forward.  The installed
transformers no longer ships the mode, so no HF code is executed here; the script runs on the CPU only.

Cases (tiny model: weight seed 31, stop bias 1.6, B = 2, Tc = 11, budget 32, repetition penalty 2.0):
  a0  (K, G, lam) = (4, 2, 1.0), lp 1.0, mode "generated", early_stopping False / True / "never"
  a1  (4, 2, 1.0), lp 0.5, "generated"         a2  (4, 2, 1.0), lp 1.0, "4.33"
  a3  (4, 2, 1.0), lp 1.0, "generated", with processors (min_new_tokens, no_repeat_ngram_size)
  b0  (4, 4, 0.5), lp 1.0, "generated"         b1  (4, 4, 0.5), lp 0.5, "4.33"
  c0  (6, 3, 1.0), lp 1.0, "generated"         c1  (6, 3, 1.0), lp 0.5, "generated"
  d   full size (weight seed 3), B = 1, Tc = 12, (4, 2, 1.0), lp 1.0, "generated"
Every run stores the ids and scores for num_return_sequences = 1 and = K, min_gap and order_gap.  The input seed of a case is searched
until every run of the case passes both screens (min_gap >= 1e-3, order_gap >= 1e-3).  The case set as a whole must show, and the
script asserts: a group that is done while another of its item still runs; an item whose returned K rows come from more than one
group; ids that differ from the plain K-beam N-best of the same inputs."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
import beam_oracle as BO                  # noqa: E402
import group_beam_oracle as GO            # noqa: E402
import nbest_oracle as NO                 # noqa: E402

TAGS = ["a0", "a1", "a2", "a3", "b0", "b1", "c0", "c1", "d"]
PROC = dict(min_new_tokens=6, no_repeat_ngram_size=2)


def inputs(in_seed, dims, B, Tc):
    return (synth.uniform(in_seed, "cond_latents", (B, 32, dims["d_model"]), 1.0), synth.integers(in_seed, "content_codes", (B, Tc), 256))


def make_case(tag, model_args, seed, in_seeds, B, Tc, K, G, lam, runs, max_new, rep=2.0, stop_bias=None):
    """runs: [(lp, mode, early_stopping index, processors or None)]"""
    dims = gcfg.gpt_dims(model_args)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][1025] = float(stop_bias)
    ora = BO.OracleGpt(w, dims)
    for in_seed in in_seeds:
        cond, codes = inputs(in_seed, dims, B, Tc)
        res = []
        for lp, mode, e, proc in runs:
            r = GO.group_beam_search(ora, cond, codes, K, G, lam, lp, rep, max_new, mode=mode, early_stopping=NO.EARLY[e], num_return=K,
                                     proc_kw=proc)
            if r["min_gap"] < 1e-3 or r["order_gap"] < 1e-3:
                print(f"  {tag}: in_seed {in_seed} lp {lp} {mode} early {NO.EARLY[e]!r} rejected (gap {r['min_gap']:.2e}, order gap "
                      f"{r['order_gap']:.2e})", flush=True)
                break
            r1 = GO.group_beam_search(ora, cond, codes, K, G, lam, lp, rep, max_new, mode=mode, early_stopping=NO.EARLY[e], num_return=1,
                                      proc_kw=proc)
            plain = None
            if proc is None:
                plain = NO.beam_search(ora, cond, codes, K, lp, rep, max_new, mode=mode, early_stopping=NO.EARLY[e], num_return=K)["ids"]
            res.append((lp, mode, e, proc, r, r1, plain))
        if len(res) == len(runs):
            break
    else:
        raise RuntimeError(f"{tag}: no input seed passed the screens")
    out, shows = {}, set()
    for i, (lp, mode, e, proc, r, r1, plain) in enumerate(res):
        p = f"{tag}_{i}_"
        out.update({p + "ids": r["ids"], p + "scores": r["scores"], p + "ids1": r1["ids"], p + "scores1": r1["scores"],
                    p + "min_gap": np.float64(r["min_gap"]), p + "order_gap": np.float64(r["order_gap"]), p + "lp": np.float64(lp),
                    p + "mode": np.array(mode), p + "early": np.int64(e), p + "proc": np.array(json.dumps(proc or {})),
                    p + "row_groups": r["row_groups"], p + "steps": np.int64(r["steps"])})
        if r["staggered"]:
            shows.add("staggered")
        if any(len(set(r["row_groups"][b * K:(b + 1) * K].tolist())) > 1 for b in range(B)):
            shows.add("mixed")
        if plain is not None and (plain.shape != r["ids"].shape or not np.array_equal(plain, r["ids"])):
            shows.add("diverse")
    out.update({f"{tag}_seed": np.int64(seed), f"{tag}_in_seed": np.int64(in_seed), f"{tag}_B": np.int64(B), f"{tag}_Tc": np.int64(Tc),
                f"{tag}_K": np.int64(K), f"{tag}_G": np.int64(G), f"{tag}_lam": np.float64(lam), f"{tag}_n": np.int64(len(res)),
                f"{tag}_rep": np.float64(rep), f"{tag}_max_new": np.int64(max_new),
                f"{tag}_stop_bias": np.float64(stop_bias if stop_bias is not None else 0.0),
                f"{tag}_full": np.int64(model_args is gcfg.DEFAULT_MODEL_ARGS), f"{tag}_shows": np.array(sorted(shows))})
    print(f"{tag}: in_seed {in_seed}, {len(res)} runs, shows {sorted(shows)}, steps {[int(x[4]['steps']) for x in res]}, min gap "
          f"{min(x[4]['min_gap'] for x in res):.2e}, order gap {min(x[4]['order_gap'] for x in res):.2e}", flush=True)
    return out


def main():
    torch.manual_seed(0)
    # one thread by default: the restatement's fp32 sums (the stored scores and gaps) then do not depend on the host's core count
    torch.set_num_threads(int(os.environ.get("GROUP_BEAM_THREADS", "1")))
    tiny = dict(model_args=gcfg.TINY_MODEL_ARGS, seed=31, B=2, Tc=11, max_new=32, stop_bias=1.6)
    G, F, T, NV = "generated", 0, 1, 2
    cases = {
        "a0": dict(tiny, in_seeds=range(5000, 5400), K=4, G=2, lam=1.0, runs=[(1.0, G, F, None), (1.0, G, T, None), (1.0, G, NV, None)]),
        "a1": dict(tiny, in_seeds=range(5000, 5400), K=4, G=2, lam=1.0, runs=[(0.5, G, F, None)]),
        "a2": dict(tiny, in_seeds=range(5000, 5400), K=4, G=2, lam=1.0, runs=[(1.0, "4.33", F, None)]),
        "a3": dict(tiny, in_seeds=range(5000, 5400), K=4, G=2, lam=1.0, runs=[(1.0, G, F, PROC)]),
        "b0": dict(tiny, in_seeds=range(5000, 5400), K=4, G=4, lam=0.5, runs=[(1.0, G, F, None)]),
        "b1": dict(tiny, in_seeds=range(5000, 5400), K=4, G=4, lam=0.5, runs=[(0.5, "4.33", F, None)]),
        "c0": dict(tiny, in_seeds=range(5000, 5600), K=6, G=3, lam=1.0, runs=[(1.0, G, F, None)]),
        "c1": dict(tiny, in_seeds=range(5000, 5600), K=6, G=3, lam=1.0, runs=[(0.5, G, F, None)]),
        "d": dict(model_args=gcfg.DEFAULT_MODEL_ARGS, seed=3, in_seeds=range(300, 340), B=1, Tc=12, K=4, G=2, lam=1.0,
                  runs=[(1.0, G, F, None)], max_new=32),
    }
    only = os.environ.get("GROUP_BEAM_ONLY", ",".join(TAGS)).split(",")
    out = {}
    for tag in TAGS:
        if tag in only:
            out.update(make_case(tag, rep=2.0, **cases[tag]))
    path = os.path.join(ROOT, "tests", "golden", "group_beam.npz")
    if only != TAGS and os.path.exists(path):
        out = dict(dict(np.load(path)), **out)
    shows = set()
    for tag in TAGS:
        shows |= set(out[f"{tag}_shows"].tolist())
    assert {"staggered", "mixed", "diverse"} <= shows, f"the case set shows only {sorted(shows)}"
    np.savez_compressed(path, **out)
    print(f"wrote {path}: shows {sorted(shows)}")


if __name__ == "__main__":
    main()
