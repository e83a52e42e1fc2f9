"""Cost of deterministic beam search on one MI355X: configs[1]'s segment shape at full size (GenVC_small dims, synthetic
weights, one 1 s segment = 13 content codes -> a 48-row prompt, 24 tokens per segment as in bench.py's headline), non-streaming.

    python scripts/bench_beam.py [--out profiles/beam_bench.json] [--reps 5]

Per beam width K in {1 (the greedy path of today), 2, 4}:
  * ms_per_step: device time of the decode loop (GPT.generate's generate / beam_generate calls, prefill excluded) / the steps they ran
    (a beam search stops when every item is done, at a group boundary: `steps`);
  * segments_per_s and utts_per_s (10 segments per utterance, GPT only: prefix + prefill + the loop + finalisation);
  * select_us: gvc_beam_select alone, back-to-back launches between two events, on this K's logits;
  * copy_bytes_per_step and pure_permutation_share: a step-by-step run that reads each step's copy lists (fp32 KV:
    2 * n_layer * d_model * 4 bytes per copied position).
The one-launch rows step serves K = 2 and 4 (B*K rows); K = 1 is the one-stream step."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402


def build_gpt(max_slots=8):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.DEFAULT_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    dims = gcfg.gpt_dims(a)
    g.load_state_dict(synth.make_weights(1, synth.gpt_weight_spec(dims)), strict=False)
    g.to("cuda")
    g.init_gpt_for_inference(max_slots=max_slots)
    return g, dims


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from genvc_amd.engine import BeamSearch, beam_select
    g, dims = build_gpt()
    eng = g.engine
    d, L, V = dims["d_model"], dims["n_layer"], dims["num_audio_tokens"]
    n_new = 24
    cond = synth.uniform(300, "cond_latents", (1, 32, d), 1.0).cuda()
    codes = synth.integers(300, "content_codes", (1, 13), 256).cuda()
    n0 = 32 + 13 + 3
    eng.warmup(1, n0 + n_new, 1)
    eng.warmup_range(1, n0 + 1, n0 + n_new, 1)
    for K in (2, 4):
        eng.warmup_beam(1, K, n0 + n_new)
    lazy0 = eng.lazy_inits()
    res = dict(workload="configs[1] segment shape, full size (L=%d d=%d), 1 s segment = 13 codes, prompt %d, %d tokens per segment, "
                        "non-streaming, synthetic weights, fp32" % (L, d, n0, n_new), results=[])
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for K in (1, 2, 4):
        kw = dict(top_k=1, repetition_penalty=2.0, max_new_tokens=n_new, group=8) if K == 1 else \
            dict(num_beams=K, do_sample=False, repetition_penalty=2.0, max_new_tokens=n_new, group=8)
        # loop-only device time: the engine's generate / beam_generate calls between two events
        loop_ms, loop_steps = [], []
        orig = eng.generate if K == 1 else eng.beam_generate

        def timed(*a, **k):
            ev0.record()
            orig(*a, **k)
            ev1.record()
            ev1.synchronize()
            loop_ms.append(ev0.elapsed_time(ev1))
            loop_steps.append(int(a[6] if K == 1 else a[2]))          # (generate's n_steps / beam_generate's n_steps)
        if K == 1:
            eng.generate = timed
        else:
            eng.beam_generate = timed
        g.generate(cond, codes, **kw)                     # (warm)
        loop_ms.clear()
        loop_steps.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            out = g.generate(cond, codes, **kw)
        torch.cuda.synchronize()
        seg_s = (time.perf_counter() - t0) / args.reps
        if K == 1:
            del eng.generate
        else:
            del eng.beam_generate
        steps = sum(loop_steps) / args.reps                 # (a search whose items are all done stops early, at a group boundary)
        row = dict(K=K, steps=steps, ms_per_step=sum(loop_ms) / sum(loop_steps), segment_ms=seg_s * 1e3, segments_per_s=1.0 / seg_s,
                   utts_per_s=1.0 / (10 * seg_s), tokens=int(out.shape[1]), decode_variant=eng.decode_variant())
        if K > 1:
            # select alone, on real logits
            fake = g.compute_embeddings(cond, codes)
            beam = BeamSearch(fake, K, n_new, 1025, V, 1.0, 2.0)
            logits = torch.randn(K, V, device="cuda")
            sl = torch.arange(K, device="cuda", dtype=torch.int32)
            beam_select(beam, logits, sl, 0)
            n = 200
            ev0.record()
            for _ in range(n):
                beam.done.zero_()
            ev1.record()
            ev1.synchronize()
            zero_ms = ev0.elapsed_time(ev1)
            ev0.record()
            for _ in range(n):
                beam.done.zero_()
                beam_select(beam, logits, sl, 0)
            ev1.record()
            ev1.synchronize()
            row["select_us"] = (ev0.elapsed_time(ev1) - zero_ms) / n * 1e3
            # copies, step by step
            slots = torch.arange(K, device="cuda", dtype=torch.int32)
            eng.prefill(slots[::K].contiguous(), g._prefix, want_outputs=False)
            beam = BeamSearch(fake, K, n_new, 1025, V, 1.0, 2.0)
            per_pos = 2 * L * d * 4
            bytes_, pure = [], 0
            for t in range(n_new):
                eng.beam_generate(slots, beam, 1, max_keys=n0 + t + 1)
                nc = int(beam.n_copies[0])
                span = n0 if t == 0 else t                   # positions [lo, cur): the prefix at the first step, the generated ones after
                bytes_.append(nc * span * per_pos)
                pure += nc == 0
            row.update(copy_bytes_per_step_mean=sum(bytes_) / len(bytes_), copy_bytes_first_step=bytes_[0],
                       copy_bytes_per_step_after_first=sum(bytes_[1:]) / max(1, len(bytes_) - 1),
                       pure_permutation_share=pure / n_new, kv_bytes_per_position_per_beam=per_pos)
        res["results"].append(row)
        print(json.dumps(row))
    res["lazy_inits_after_warmup"] = eng.lazy_inits() - lazy0
    res["note"] = ("ms_per_step = device time of the loop calls / steps (greedy K = 1: sample + one-stream step; K > 1: select + span "
                   "copies + B*K-row step); select_us from back-to-back gvc_beam_select launches minus the same loop without them; "
                   "the span copies are not timed separately (no rocprofv3 run)")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
