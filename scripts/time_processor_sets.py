"""Per-row processor sets against one call-wide set, on full-size synthetic weights.

    rocprofv3 --kernel-trace --stats -- python scripts/time_processor_sets.py --mode kernels --sets wide|rows
        16 streams, 24 greedy (k_sample_greedy) and 24 top_k 15 (k_sample) steps per rep: one set for every row (gvc_gpt_generate_proc)
        or 4 distinct sets over the rows plus rows without one (gvc_gpt_generate_proc_sets), for the per-launch kernel times.
    python scripts/time_processor_sets.py --mode calls [--out profiles/processor_sets.json]
        the host cost per generate call of staging 1, 4 and 16 sets (B = 16, 8 greedy steps per call) against the call-wide set, and
        ms per scheduling step of an 8-session StreamSessions decode with 4 distinct sets against none."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_beam import build_gpt          # noqa: E402
from genvc_amd import synth               # noqa: E402
from genvc_amd.engine import logits_processor_sets, logits_processors, sample_params   # noqa: E402

EOS, V = 1025, 1026
SETS = [dict(no_repeat_ngram_size=3, suppress_tokens=[3]), dict(min_new_tokens=8, begin_suppress_tokens=[5]),
        dict(exponential_decay_length_penalty=(10, 1.05), suppress_tokens=[700]), dict(min_length=60, min_p=0.05)]


def _state(eng, prefix, n):
    B, P = prefix.shape[0], prefix.shape[1]
    slots = torch.arange(B, device="cuda", dtype=torch.int32)
    eng.prefill(slots, prefix, want_outputs=False)
    ids = torch.ones(B, P + 1 + n + 8, device="cuda", dtype=torch.int32)
    ids[:, P] = eng.dims["start_audio_token"]
    return (slots, ids, torch.full((B,), P + 1, device="cuda", dtype=torch.int32), torch.zeros(B, device="cuda", dtype=torch.int32),
            torch.full((B, n), EOS, device="cuda", dtype=torch.int32), torch.empty(B, n, eng.d, device="cuda"), P)


def _decode(eng, prefix, top_k, n, group, wide=None, sets=None):
    slots, ids, ids_len, fin, toks, lats, P = _state(eng, prefix, n)
    params = sample_params(dict(repetition_penalty=2.0, temperature=0.85, top_p=0.85, top_k=top_k), V, EOS, seed=3)
    for i0 in range(0, n, group):
        if sets is not None:
            eng.generate_proc_sets(slots, ids, ids_len, fin, params, sets, i0, group, toks, lats, max_keys=P + 1 + i0 + group)
        else:
            eng.generate(slots, ids, ids_len, fin, params, i0, group, toks, lats, max_keys=P + 1 + i0 + group, proc=wide)


def kernels(g, dims, which, reps):
    B = 16
    eng = g.engine
    cond = synth.uniform(300, "cond_latents", (B, 32, dims["d_model"]), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (B, 13), 256).cuda().int()
    prefix = eng.prefix_embeddings(cond, codes)
    P = prefix.shape[1]
    wide = logits_processors(dict(SETS[0], **SETS[1]), P + 1, V)
    rows = logits_processor_sets([SETS[b % 5] if b % 5 < 4 else None for b in range(B)], P + 1, V)
    for _ in range(reps):
        for top_k in (1, 15):
            if which == "wide":
                _decode(eng, prefix, top_k, 24, 8, wide=wide)
            else:
                _decode(eng, prefix, top_k, 24, 8, sets=rows)
    torch.cuda.synchronize()


def calls(g, dims, reps, out):
    B = 16
    eng = g.engine
    cond = synth.uniform(300, "cond_latents", (B, 32, dims["d_model"]), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (B, 13), 256).cuda().int()
    prefix = eng.prefix_embeddings(cond, codes)
    P = prefix.shape[1]
    wide = logits_processors(SETS[0], P + 1, V)
    variants = {"none": {}, "wide": dict(wide=wide)}
    for n in (1, 4, 16):
        kws = [dict(suppress_tokens=[3 + (b % n)], no_repeat_ngram_size=3) for b in range(B)]
        variants[f"sets{n}"] = dict(sets=logits_processor_sets(kws, P + 1, V))
    res = {}
    for name, kw in variants.items():
        _decode(eng, prefix, 1, 8, 8, **kw)                 # warm
        torch.cuda.synchronize()
        t = []
        for _ in range(reps):
            slots, ids, ids_len, fin, toks, lats, _ = _state(eng, prefix, 8)
            params = sample_params(dict(repetition_penalty=2.0, temperature=1.0, top_p=1.0, top_k=1), V, EOS)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if "sets" in kw:
                eng.generate_proc_sets(slots, ids, ids_len, fin, params, kw["sets"], 0, 8, toks, lats, max_keys=P + 9)
            else:
                eng.generate(slots, ids, ids_len, fin, params, 0, 8, toks, lats, max_keys=P + 9, proc=kw.get("wide"))
            t1 = time.perf_counter()                    # host: the call's enqueue
            torch.cuda.synchronize()
            t.append(((t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6))
        t.sort(key=lambda x: x[1])
        mid = t[len(t) // 2]
        res[name] = dict(enqueue_us=round(sorted(x[0] for x in t)[len(t) // 2], 1), call_us=round(mid[1], 1))
        print(name, res[name], flush=True)
    res["sessions_ms_per_step"] = sessions(reps)
    if out:
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


def sessions(reps):
    """8 sessions, one 2 s segment each, greedy: ms per StreamSessions.step() while all decode, 4 distinct sets (2 sessions each) vs none"""
    from genvc_amd import config as gcfg
    from genvc_amd.inference.inference_utils import segments
    from genvc_amd.inference.model_init import model_init_synthetic
    from genvc_amd.streaming import StreamSessions
    m = model_init_synthetic(gcfg.default_config(), seed=5, device="cuda", max_slots=8)[0]
    m.config.top_k = 1
    m.gpt.max_gen_mel_tokens = 64
    refs = [synth.synth_audio(60 + i, "ref", 72000) for i in range(8)]
    src = synth.synth_audio(80, "src", 32000)
    seg = list(segments(src, 16000, 32000))[0]
    out = {}
    for name in ("none", "sets4", "none", "sets4"):
        ss = StreamSessions(m, max_sessions=8, group=8)
        for i in range(8):
            sid = ss.open(refs[i], generate_kwargs=SETS[i % 4] if name == "sets4" else None)
            ss.push(sid, seg)
        ss.step()                                           # the prefills and the first decode call
        torch.cuda.synchronize()
        t = []
        for _ in range(min(reps, 6)):
            t0 = time.perf_counter()
            ss.step()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        out.setdefault(name, []).append(round(sorted(t)[len(t) // 2], 3))
        print("sessions", name, out[name], flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernels", "calls"], required=True)
    ap.add_argument("--sets", choices=["wide", "rows"], default="rows")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    g, dims = build_gpt(max_slots=16)
    if args.mode == "kernels":
        kernels(g, dims, args.sets, args.reps)
    else:
        calls(g, dims, args.reps, args.out)
    print("done", args.mode)


if __name__ == "__main__":
    main()
