"""tests/golden/beam_search.npz: the reference's `GPT.generate(num_beams=K, do_sample=False)` (layers/gpt.py:594-609) EXECUTED on the
reference classes, with the installed transformers' `_beam_search` behind it (the reference pins 4.33, whose generation code is not
installed here: DESIGN.md 4.7).  Four shims make the reference's GPT2InferenceModel generate under transformers 5, and nothing else:
  * its class also inherits GenerationMixin and it carries a default GenerationConfig();
  * config.vocab_size = 1026 (the audio vocabulary the mel head scores);
  * prepare_inputs_for_generation passes past_key_values=None while the cache is empty (transformers 5 hands an empty DynamicCache to
    the first step, which would make the reference slice the prompt away);
  * _reorder_cache calls past.reorder_cache(beam_idx): the reference's index_select on the batch dim (gpt_inference.py:126-136),
    applied to a Cache object.
Each case stores its inputs' seeds, the returned ids and the best score per item, plus the margin screen the tests re-assert (every
K-th vs (K+1)-th non-EOS gap and every EOS-vs-worst comparison >= 1e-3), computed by the CPU restatement (tests/beam_oracle.py) on the
oracle's GPT forward."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG      # noqa: E402
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
import beam_oracle as BO                  # noqa: E402


def arm_beam(g):
    from transformers import GenerationConfig, GenerationMixin
    gi = g.gpt_inference
    base = type(gi)

    class BeamInference(base, GenerationMixin):
        def prepare_inputs_for_generation(self, input_ids, past_key_values=None, **kw):
            if past_key_values is not None and past_key_values.get_seq_length() == 0:
                past_key_values = None
            kw.pop("next_sequence_length", None)
            return base.prepare_inputs_for_generation(self, input_ids, past_key_values=past_key_values, **kw)

        @staticmethod
        def _reorder_cache(past, beam_idx):
            past.reorder_cache(beam_idx)
            return past
    gi.__class__ = BeamInference
    gi.generation_config = GenerationConfig()
    gi.config.vocab_size = 1026
    return g


def ref_beam(g, cond, codes, K, lp, rep, max_new):
    g.max_gen_mel_tokens = max_new
    with torch.inference_mode():
        out = g.generate(cond, codes, num_beams=K, do_sample=False, length_penalty=lp, repetition_penalty=rep,
                         num_return_sequences=1, output_attentions=False)
    return out.numpy()


def make_case(GPT, tag, model_args, seed, in_seeds, B, Tc, K, lps, rep, max_new, stop_bias=None, need_ragged=False):
    dims = gcfg.gpt_dims(model_args)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][1025] = float(stop_bias)
    g = arm_beam(MG.build_ref_gpt(GPT, model_args, w))
    ora = BO.OracleGpt(w, dims)
    for in_seed in in_seeds:
        cond, codes = MG.gpt_inputs(in_seed, dims, B, Tc)
        res, ok = [], True
        for lp in lps:
            ids = ref_beam(g, cond, codes, K, lp, rep, max_new)
            r = BO.beam_search(ora, cond, codes, K, lp, rep, max_new, mode="generated")
            if r["min_gap"] < 1e-3 or not np.array_equal(r["ids"], ids):
                print(f"  {tag}: in_seed {in_seed} lp {lp} rejected (gap {r['min_gap']:.2e}, equal {np.array_equal(r['ids'], ids)})")
                ok = False
                break
            res.append((lp, ids, r))
        if ok and need_ragged:
            lens = [(np.asarray(ids) == 1025).argmax(1) for _, ids, _ in res]
            ok = len({tuple(x) for x in lens}) >= 1 and any(len(set(x.tolist())) > 1 for x in lens) and \
                len({ids.tobytes() for _, ids, _ in res}) > 1
            if not ok:
                print(f"  {tag}: in_seed {in_seed} not ragged / lp-dependent")
        if ok:
            break
    else:
        raise RuntimeError(f"{tag}: no input seed passed the screen")
    out = {}
    for i, (lp, ids, r) in enumerate(res):
        p = f"{tag}_{i}_"
        out.update({p + "ids": ids, p + "best_scores": r["best_scores"], p + "min_gap": np.float64(r["min_gap"]),
                    p + "lp": np.float64(lp)})
    out.update({f"{tag}_seed": np.int64(seed), f"{tag}_in_seed": np.int64(in_seed), f"{tag}_B": np.int64(B), f"{tag}_Tc": np.int64(Tc),
                f"{tag}_K": np.int64(K), f"{tag}_n": np.int64(len(res)), f"{tag}_rep": np.float64(rep), f"{tag}_max_new": np.int64(max_new),
                f"{tag}_stop_bias": np.float64(stop_bias if stop_bias is not None else 0.0),
                f"{tag}_full": np.int64(model_args is gcfg.DEFAULT_MODEL_ARGS)})
    print(f"{tag}: in_seed {in_seed}, ids {[r[1].shape for r in res]}, min gap {min(r[2]['min_gap'] for r in res):.2e}")
    return out


def main():
    torch.manual_seed(0)
    GPT, _ = MG.import_reference()
    out = {}
    tiny = gcfg.TINY_MODEL_ARGS
    out.update(make_case(GPT, "a", tiny, 29, range(2950, 2990), B=2, Tc=9, K=4, lps=[1.0], rep=2.0, max_new=24))
    out.update(make_case(GPT, "b", tiny, 31, range(3100, 3160), B=3, Tc=11, K=3, lps=[0.5, 1.0, 2.0], rep=2.0, max_new=40,
                         stop_bias=float(os.environ.get("BEAM_STOP_BIAS", "1.6")), need_ragged=True))
    if os.environ.get("BEAM_FULL", "1") == "1":
        out.update(make_case(GPT, "c", gcfg.DEFAULT_MODEL_ARGS, 3, range(300, 320), B=1, Tc=12, K=4, lps=[1.0], rep=2.0, max_new=40))
    np.savez_compressed(os.path.join(MG.GOLD, "beam_search.npz"), **out)


if __name__ == "__main__":
    main()
