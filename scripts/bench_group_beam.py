"""Cost of group (diverse) beam search on one MI355X at the shape of scripts/bench_beam.py: full size, one 1 s segment
= 13 content codes -> a 48-row prompt, 24 steps, K = 4 beams, non-streaming, synthetic weights, fp32.

    python scripts/bench_group_beam.py [--out profiles/group_beam_bench.json] [--reps 5]

Per G in {1 (the plain search through gvc_gpt_beam_generate), 2, 4 (gvc_gpt_group_beam_generate)}:
  * ms_per_step: device time of the loop calls (prefill excluded; G > 1: the first call's prefix fan-out included) / the steps they ran;
  * select_us: the select launch alone (gvc_beam_select for G = 1, gvc_group_beam_select for G > 1), back-to-back launches between two
    events on this K's logits, minus the same loop without them;
  * copy_bytes_per_step: a step-by-step run that reads each step's copy lists (fp32 KV: 2 * n_layer * d_model * 4 bytes per copied
    position); fanout_bytes: the K - 1 whole prefixes a G > 1 search copies before its first step."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from genvc_amd import synth               # noqa: E402
from bench_beam import build_gpt          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_beam_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from genvc_amd.engine import BeamSearch, GroupBeamSearch, beam_select, group_beam_select
    g, dims = build_gpt()
    eng = g.engine
    d, L, V = dims["d_model"], dims["n_layer"], dims["num_audio_tokens"]
    n_new, K, lam = 24, 4, 1.0
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    n0 = 32 + 13 + 3
    eng.warmup_beam(1, K, n0 + n_new)
    eng.warmup_group_beam(1, K, 2, n0 + n_new)
    lazy0 = eng.lazy_inits()
    res = dict(workload="configs[1] segment shape, full size (L=%d d=%d), 1 s segment = 13 codes, prompt %d, %d steps, K = %d, "
                        "diversity_penalty %g, non-streaming, synthetic weights, fp32" % (L, d, n0, n_new, K, lam), results=[])
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per_pos = 2 * L * d * 4
    for G in (1, 2, 4):
        kw = dict(num_beams=K, do_sample=False, repetition_penalty=2.0, max_new_tokens=n_new, group=8)
        if G > 1:
            kw.update(num_beam_groups=G, diversity_penalty=lam)
        name = "beam_generate" if G == 1 else "group_beam_generate"
        loop_ms, loop_steps = [], []
        orig = getattr(eng, name)

        def timed(*a, **k):
            ev0.record()
            orig(*a, **k)
            ev1.record()
            ev1.synchronize()
            loop_ms.append(ev0.elapsed_time(ev1))
            loop_steps.append(int(a[2]))
        setattr(eng, name, timed)
        g.generate(cond, codes, **kw)                     # (warm)
        loop_ms.clear()
        loop_steps.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            out = g.generate(cond, codes, **kw)
        torch.cuda.synchronize()
        seg_s = (time.perf_counter() - t0) / args.reps
        delattr(eng, name)
        row = dict(K=K, G=G, entry="gvc_gpt_" + name, steps=sum(loop_steps) / args.reps, ms_per_step=sum(loop_ms) / sum(loop_steps),
                   segment_ms=seg_s * 1e3, tokens=int(out.shape[1]), decode_variant=eng.decode_variant())
        # the select launch alone
        fake = g.compute_embeddings(cond, codes)
        mk = (lambda: BeamSearch(fake, K, n_new, 1025, V, 1.0, 2.0)) if G == 1 else \
            (lambda: GroupBeamSearch(fake, K, G, lam, n_new, 1025, V, 1.0, 2.0))
        sel = beam_select if G == 1 else group_beam_select
        beam = mk()
        logits = torch.randn(K, V, device="cuda")
        sl = torch.arange(K, device="cuda", dtype=torch.int32)
        flags = beam.done if G == 1 else beam.group_done
        sel(beam, logits, sl, 0)
        n = 200
        ev0.record()
        for _ in range(n):
            flags.zero_()
        ev1.record()
        ev1.synchronize()
        zero_ms = ev0.elapsed_time(ev1)
        ev0.record()
        for _ in range(n):
            flags.zero_()
            sel(beam, logits, sl, 0)
        ev1.record()
        ev1.synchronize()
        row["select_us"] = (ev0.elapsed_time(ev1) - zero_ms) / n * 1e3
        # copies, step by step
        slots = torch.arange(K, device="cuda", dtype=torch.int32)
        eng.prefill(slots[::K].contiguous(), g._prefix, want_outputs=False)
        beam = mk()
        bytes_, pure = [], 0
        for t in range(n_new):
            getattr(eng, name)(slots, beam, 1, max_keys=n0 + t + 1)
            nc = int(beam.n_copies[0])
            span = n0 if (t == 0 and G == 1) else t           # G > 1: the prefix went out with the fan-out, spans start at n0
            bytes_.append(nc * span * per_pos)
            pure += nc == 0
        row.update(copy_bytes_per_step_mean=sum(bytes_) / len(bytes_), copy_bytes_per_step_after_first=sum(bytes_[1:]) / (len(bytes_) - 1),
                   fanout_bytes=0 if G == 1 else (K - 1) * n0 * per_pos, pure_permutation_share=pure / n_new,
                   kv_bytes_per_position_per_beam=per_pos)
        res["results"].append(row)
        print(json.dumps(row), flush=True)
    res["lazy_inits_after_warmup"] = eng.lazy_inits() - lazy0
    res["note"] = ("ms_per_step = device time of the loop calls / steps (select + span copies + 4-row decode step; G > 1 also the one "
                   "prefix fan-out of the first call); select_us from back-to-back select launches minus the same loop without them")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
