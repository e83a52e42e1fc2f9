"""tests/golden/nbest.npz: the reference's `GPT.generate(num_beams=K, do_sample=False, num_return_sequences=N, early_stopping=...)`
(layers/gpt.py:594-609 forwards every kwarg to HF generate) EXECUTED on the reference classes under the installed transformers, through
the shims of scripts/make_beam_golden.py (arm_beam) and the helpers of oracle/make_golden.py.

Cases: a0 a1 a2  tiny, B = 3, K = 3, N in {2, 3};  b0 b1  tiny, B = 2, K = 4, N = 2;  c  full size, B = 1, K = 4, N = 4 -- each with
early_stopping in {False, True, "never"} and the length penalty listed in main().  NBEST_ONLY=a1,c regenerates those cases alone and
keeps the others of the file.  Input seeds are searched until every run of a case passes the
margin screens -- the existing one (every K-th vs (K+1)-th non-EOS gap and every comparison with the worst kept score >= 1e-3) and the
order screen (the kept hypotheses' normalised scores pairwise >= 1e-3 apart) -- with the CPU restatement (tests/nbest_oracle.py)
returning the executed ids, and until the case set as a whole matters: the ids under True differ from those under False somewhere, the
ids under "never" differ from those under False somewhere (length_penalty > 0), and rows end at different steps somewhere.  Each run
stores its ids, the restatement's scores and both gaps; the tests re-assert the gaps."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from oracle import make_golden as MG      # noqa: E402
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
import beam_oracle as BO                  # noqa: E402
import nbest_oracle as NO                 # noqa: E402
from make_beam_golden import arm_beam     # noqa: E402


def ref_nbest(g, cond, codes, K, N, lp, rep, early, max_new):
    g.max_gen_mel_tokens = max_new
    with torch.inference_mode():
        out = g.generate(cond, codes, num_beams=K, do_sample=False, length_penalty=lp, repetition_penalty=rep, num_return_sequences=N,
                         early_stopping=early, output_attentions=False)
    return out.numpy()


def make_case(GPT, tag, model_args, seed, in_seeds, B, Tc, K, runs, max_new, rep=2.0, stop_bias=None, need=()):
    """runs: [(N, lp)], each executed under the three early_stopping modes.  need: subset of {"true", "never", "ragged"} the case must
    show on its own"""
    dims = gcfg.gpt_dims(model_args)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][1025] = float(stop_bias)
    g = arm_beam(MG.build_ref_gpt(GPT, model_args, w))
    ora = BO.OracleGpt(w, dims)
    for in_seed in in_seeds:
        cond, codes = MG.gpt_inputs(in_seed, dims, B, Tc)
        res, ok = [], True
        for N, lp in runs:
            for e, early in enumerate(NO.EARLY):
                ids = ref_nbest(g, cond, codes, K, N, lp, rep, early, max_new)
                r = NO.beam_search(ora, cond, codes, K, lp, rep, max_new, mode="generated", early_stopping=early, num_return=N)
                same = r["ids"].shape == ids.shape and np.array_equal(r["ids"], ids)
                if r["min_gap"] < 1e-3 or r["order_gap"] < 1e-3 or not same:
                    print(f"  {tag}: in_seed {in_seed} N {N} lp {lp} early {early!r} rejected (gap {r['min_gap']:.2e}, order gap "
                          f"{r['order_gap']:.2e}, equal {same})", flush=True)
                    ok = False
                    break
                res.append((N, lp, e, ids, r))
            if not ok:
                break
        if not ok:
            continue
        by = {(N, lp, e): ids for N, lp, e, ids, _ in res}
        differs = lambda e: any(by[(N, lp, e)].shape != by[(N, lp, 0)].shape or not np.array_equal(by[(N, lp, e)], by[(N, lp, 0)])
                                for N, lp in runs)          # noqa: E731
        have = set()
        if differs(1):
            have.add("true")
        if any(lp > 0 for _, lp in runs) and differs(2):
            have.add("never")
        for _, _, _, ids, _ in res:
            ends = [int((row == 1025).argmax()) if (row == 1025).any() else ids.shape[1] for row in ids]
            if len(set(ends)) > 1:
                have.add("ragged")
        if set(need) <= have:
            break
        print(f"  {tag}: in_seed {in_seed} shows {sorted(have)}, needs {sorted(need)}", flush=True)
    else:
        raise RuntimeError(f"{tag}: no input seed passed the screens")
    out = {}
    for i, (N, lp, e, ids, r) in enumerate(res):
        p = f"{tag}_{i}_"
        out.update({p + "ids": ids, p + "scores": r["scores"], p + "min_gap": np.float64(r["min_gap"]),
                    p + "order_gap": np.float64(r["order_gap"]), p + "lp": np.float64(lp), p + "N": np.int64(N), p + "early": np.int64(e)})
    out.update({f"{tag}_seed": np.int64(seed), f"{tag}_in_seed": np.int64(in_seed), f"{tag}_B": np.int64(B), f"{tag}_Tc": np.int64(Tc),
                f"{tag}_K": np.int64(K), f"{tag}_n": np.int64(len(res)), f"{tag}_rep": np.float64(rep), f"{tag}_max_new": np.int64(max_new),
                f"{tag}_stop_bias": np.float64(stop_bias if stop_bias is not None else 0.0),
                f"{tag}_full": np.int64(model_args is gcfg.DEFAULT_MODEL_ARGS), f"{tag}_shows": np.array(sorted(have))})
    print(f"{tag}: in_seed {in_seed}, {len(res)} runs, shows {sorted(have)}, min gap {min(r['min_gap'] for *_, r in res):.2e}, "
          f"order gap {min(r['order_gap'] for *_, r in res):.2e}", flush=True)
    return out


def main():
    torch.manual_seed(0)
    # one thread by default: the restatement's fp32 sums (the stored scores and gaps) then do not depend on the host's core count
    torch.set_num_threads(int(os.environ.get("NBEST_THREADS", "1")))
    GPT, _ = MG.import_reference()
    out = {}
    tiny = gcfg.TINY_MODEL_ARGS
    only = os.environ.get("NBEST_ONLY", ",".join(NO.TAGS)).split(",")
    # (one input seed per (N, length_penalty) of a shape: a seed has to pass the screens under all three early_stopping modes at once)
    cases = {
        "a0": dict(model_args=tiny, seed=31, in_seeds=range(3100, 3400), B=3, Tc=11, K=3, runs=[(2, 1.0)], max_new=40, stop_bias=1.6,
                   need=("never", "ragged")),
        "a1": dict(model_args=tiny, seed=31, in_seeds=range(3400, 4000), B=3, Tc=11, K=3, runs=[(3, 1.0)], max_new=40, stop_bias=1.6),
        "a2": dict(model_args=tiny, seed=31, in_seeds=range(4000, 4300), B=3, Tc=11, K=3, runs=[(2, 0.5)], max_new=40, stop_bias=1.6),
        "b0": dict(model_args=tiny, seed=29, in_seeds=range(2950, 3250), B=2, Tc=9, K=4, runs=[(2, 1.0)], max_new=24, stop_bias=1.6,
                   need=("true",)),
        # (length_penalty 2 divides by len ** 2: kept scores 1e-3 apart need short hypotheses, hence the stronger stop bias and the
        #  smaller budget; no seed of 600 passed the screens at B = 3, K = 3 with it)
        "b1": dict(model_args=tiny, seed=29, in_seeds=range(3600, 3850), B=2, Tc=9, K=4, runs=[(2, 2.0)], max_new=12, stop_bias=3.0),
        "c": dict(model_args=gcfg.DEFAULT_MODEL_ARGS, seed=3, in_seeds=range(300, 340), B=1, Tc=12, K=4, runs=[(4, 1.0)], max_new=40),
    }
    for tag in NO.TAGS:
        if tag in only:
            out.update(make_case(GPT, tag, rep=2.0, **cases[tag]))
    path = os.path.join(MG.GOLD, "nbest.npz")
    if only != NO.TAGS and os.path.exists(path):
        out = dict(dict(np.load(path)), **out)
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    main()
