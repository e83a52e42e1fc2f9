"""Generate tests/golden/trace_*.npz: per-step attentions and hidden states of the reference's GPT2InferenceModel, driven step by step
as oracle.make_golden.ref_greedy drives it, with eager attention, output_attentions=True and output_hidden_states=True.

Runs only where the reference checkout is present (oracle.make_golden.import_reference); nothing of it is copied -- its classes are
imported, loaded with synthetic weights and called.

    python scripts/make_trace_golden.py [--only tiny|hd256|hd64|hd128]

Per case (tests/trace_oracle.py: CASES, SHAPES) one file with
  * the seeds, the stop-token bias of the ragged case, the greedy tokens, their top-1 / top-2 margins and the generated lengths;
  * every step's attentions (att_<step>: [L,B,H,rows,keys], rows = P + 1 at step 0 and 1 afterwards) and hidden states (hid_<step>:
    [L+1,B,rows,channels]; the d 1024 cases keep every 8th channel);
  * floor_att / floor_hid in the DESIGN 4.22 sense, from a second run of the reference in float64 over the same tokens:
    max(max|fp32 - fp64|, 2^-24 max|value|), the maximum taken over what is stored;
  * peak: per layer, the median over the stored live rows of max_k p * (number of keys) -- asserted >= 4 (trace_oracle.MIN_PEAK):
    with the default synthetic weights every softmax is near uniform and a kernel that ignored the scores would pass, so the weights
    carry tests/act_stats.py's `peaked` knob (trace_oracle.PEAKED).
Seeds are screened as make_gpt screens them: every greedy decision keeps a top-1 / top-2 margin >= 2e-3, in both precisions.  The
`tiny` case raises the stop-token bias, as make_eos does, until exactly one of its two rows ends early (ragged lengths, a zeroed tail).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.make_golden import GOLD, build_ref_gpt, import_reference      # noqa: E402
import trace_oracle as TO                                                  # noqa: E402

MAX_BYTES = 900 * 1024


@torch.inference_mode()
def ref_steps(g, cond, codes, n_steps, forced=None):
    """greedy steps of the reference's gpt_inference (repetition penalty 1, top_k 1: the argmax) that keep every step's attentions
    and hidden states; `forced` [B, n]: feed these tokens instead (the float64 run follows the float32 run's tokens)"""
    gi = g.gpt_inference
    gi.transformer.config._attn_implementation = "eager"          # the default sdpa returns an empty attentions tuple
    ids = g.compute_embeddings(cond, codes)
    stop = g.stop_audio_token
    B = ids.shape[0]
    unfinished = torch.ones(B, dtype=torch.long)
    pkv = None
    toks, margins, atts, hids = [], [], [], []
    for step in range(n_steps):
        inputs = gi.prepare_inputs_for_generation(ids, past_key_values=pkv, attention_mask=torch.ones_like(ids), use_cache=True)
        out = gi(**inputs, return_dict=True, output_attentions=True, output_hidden_states=True)
        pkv = out.past_key_values
        assert len(out.attentions) == len(gi.transformer.h) and len(out.hidden_states) == len(gi.transformer.h) + 1
        logits = out.logits[:, -1, :]
        top2 = torch.topk(logits, 2, dim=-1)[0]
        margins.append((top2[:, 0] - top2[:, 1]).double().numpy())
        nxt = logits.argmax(-1)
        nxt = nxt * unfinished + stop * (1 - unfinished)
        if forced is not None:
            nxt = forced[:, step]
        atts.append(torch.stack(out.attentions))                   # [L,B,H,rows,keys]
        hids.append(torch.stack(out.hidden_states))                # [L+1,B,rows,d]
        toks.append(nxt)
        ids = torch.cat([ids, nxt[:, None]], dim=-1)
        unfinished = unfinished * (nxt != stop).long()
    return torch.stack(toks, 1), np.stack(margins, 1), atts, hids


def live_margin(margins, lengths):
    """smallest margin over the decisions that count: step i of row b with i < lengths[b]"""
    n = margins.shape[1]
    live = np.arange(n)[None, :] < np.asarray(lengths)[:, None]
    return float(margins[live].min())


def floor_of(a32, a64):
    dev = max(float((x.double() - y).abs().max()) for x, y in zip(a32, a64))
    top = max(float(y.abs().max()) for y in a64)
    return max(dev, 2.0 ** -24 * top)


def run_case(GPT, tag, w, cond, codes, steps):
    model_args = TO.CASES[tag]
    g = build_ref_gpt(GPT, model_args, w)
    toks, margins, atts, hids = ref_steps(g, cond, codes, steps)
    g64 = build_ref_gpt(GPT, model_args, {k: v.double() for k, v in w.items()}).double()
    toks64, margins64, atts64, hids64 = ref_steps(g64, cond.double(), codes, steps, forced=toks)
    return toks, margins, margins64, atts, hids, atts64, hids64


def make_case(GPT, tag):
    sh, dims = TO.SHAPES[tag], TO.case_dims(tag)
    stop, steps = dims["stop_audio_token"], sh["steps"]
    found = None
    for seed in range(sh["seed"], sh["seed"] + 20):
        cond, codes = TO.case_inputs(tag, seed)
        biases = [float(b) for b in np.arange(0.2, 6.0, 0.1)] if sh["ragged"] else [None]
        for bias in biases:
            w = TO.case_weights(tag, seed, stop_bias=bias)
            toks, margins, margins64, atts, hids, atts64, hids64 = run_case(GPT, tag, w, cond, codes, steps)
            lengths = TO.lengths_of(toks, stop).numpy()
            if sh["ragged"]:
                ends = sorted(int(x) for x in lengths)
                if ends[-1] < steps:                    # both rows stopped: a larger bias only stops them sooner
                    break
                if not (4 <= ends[0] < steps - 2):
                    continue
            m = min(live_margin(margins, lengths), live_margin(margins64, lengths))
            if m >= TO.MIN_MARGIN:
                found = True
            else:
                print(f"  trace_{tag}: seed {seed} bias {bias} rejected (margin {m:.2e})")
            break
        if found:
            break
    else:
        raise RuntimeError("no seed passed the margin screen")
    L, d = dims["n_layer"], dims["d_model"]
    cstep = 1 if d <= 256 else TO.HIDDEN_STEP
    sub = lambda hs: [h[..., ::cstep] for h in hs]
    out = dict(seed=seed, stop_bias=np.float64(-1.0 if bias is None else bias), tokens=toks.numpy(), margins=margins, lengths=lengths,
               channel_step=cstep, floor_att=floor_of(atts, atts64), floor_hid=floor_of(sub(hids), sub(hids64)))
    for i in range(steps):
        out[f"att_{i}"] = atts[i].numpy()
        out[f"hid_{i}"] = sub(hids)[i].numpy()
    peak = TO.stored_peak_median([[a[l] for l in range(L)] for a in atts], lengths)
    assert min(peak) >= TO.MIN_PEAK, f"trace_{tag}: attention too flat at {TO.PEAKED}: per-layer median peak {peak} -- raise the knob"
    out["peak"] = np.array(peak)
    path = os.path.join(GOLD, f"trace_{tag}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print(f"trace_{tag}: seed {seed}, stop bias {bias}, lengths {lengths.tolist()}, margin {m:.2e}, peak {[round(p, 2) for p in peak]}, "
          f"floors att {out['floor_att']:.3e} hid {out['floor_hid']:.3e}, {size} bytes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    GPT, _ = import_reference()
    for tag in TO.CASES:
        if args.only in (None, tag):
            make_case(GPT, tag)


if __name__ == "__main__":
    main()
