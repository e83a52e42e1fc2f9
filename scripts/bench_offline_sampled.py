"""BASELINE configs[2]'s workload at the reference's sampling settings (top_k 15, top_p 0.85, temperature 0.85, repetition penalty 2.0;
configs/genVC_train_configs.py): 64 synthetic 10 s utterances (segments 6 s + 4 s, 141 + 94 tokens by duration), tokens only, one GPU,
micro-batches of 8 utterances (16 decode rows).  Three schedules in one process, timed alternately:
  serial  -- every class of a micro-batch decoded on its own (convert_offline's default for sampled runs);
  joint   -- the classes of a micro-batch decoded together, rows keyed per class (joint_sampling=True);
  rolling -- a rolling set of streams across micro-batches (rolling=True, joint_sampling=True).
Prints one JSON line with utterances/s per schedule and whether the three produced the same token ids.  Not the headline benchmark."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from genvc_amd import config as gcfg, synth
from genvc_amd.inference.model_init import model_init_synthetic
from genvc_amd.parallel_offline import convert_offline

N_UTT = int(os.environ.get("N_UTT", "64"))
ROUNDS = int(os.environ.get("ROUNDS", "3"))
MB = 8
SAMPLING = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0, do_sample=True, seed=1)
m, cfg = model_init_synthetic(gcfg.default_config(), seed=1, device="cuda", max_slots=2 * MB)
srcs = [synth.synth_audio(500 + i, "src", 160000) for i in range(N_UTT)]
ref = synth.synth_audio(7, "ref", 72000)
SCHEDULES = {"serial": {}, "joint": dict(joint_sampling=True), "rolling": dict(rolling=True, joint_sampling=True)}


def run(name, wavs):
    return convert_offline(m, wavs, ref, seg_len=6.0, micro_batch=MB, max_new_tokens=141, tokens_per_second=23.4375,
                           **SAMPLING, **SCHEDULES[name])


for name in SCHEDULES:                                  # warm-up / graph capture of every shape
    run(name, srcs[:MB])
torch.cuda.synchronize()
times = {name: [] for name in SCHEDULES}
toks = {}
for _ in range(ROUNDS):
    for name in SCHEDULES:                              # alternated: drift of the box hits every schedule alike
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks[name] = run(name, srcs)
        torch.cuda.synchronize()
        times[name].append(time.perf_counter() - t0)
same = all(torch.equal(toks[name], toks["serial"]) for name in SCHEDULES)
out = {name: {"utterances_per_s": N_UTT / statistics.median(ts), "seconds": [round(t, 4) for t in ts]} for name, ts in times.items()}
print(json.dumps({"workload": f"{N_UTT} x 10 s utterances, segments 6 s + 4 s, 141 + 94 tokens, top_k=15 top_p=0.85 temperature=0.85 "
                              f"repetition_penalty=2.0, micro-batch {MB}, tokens only",
                  "n_gpus": 1, "rounds": ROUNDS, "same_token_ids": same,
                  "joint_over_serial": out["joint"]["utterances_per_s"] / out["serial"]["utterances_per_s"],
                  "rolling_over_serial": out["rolling"]["utterances_per_s"] / out["serial"]["utterances_per_s"], **out}))
if not same:
    sys.exit(1)
