"""tests/golden/logits_processors.npz: the length / repetition logits processors (min_new_tokens, min_length, no_repeat_ngram_size,
suppress_tokens, begin_suppress_tokens, exponential_decay_length_penalty) EXECUTED on the reference classes under the installed
transformers.
  * Sampler cases: the reference's own `NewGenerationMixin.sample_stream` (layers/stream_generator.py), unmodified, driven as
    oracle/make_golden.py drives it, with the processor list the installed `GenerationMixin._get_logits_processor` builds for a
    GenerationConfig carrying the kwargs (do_sample=True, top_k=1: one candidate survives, so the draw is the argmax).
  * Beam cases: the reference's `GPT.generate(num_beams=K, do_sample=False, ...)` with the shims of scripts/make_beam_golden.py.
Every case is screened: its ids must differ from the same case without the processor kwargs, and from the same case without any ONE
of them (each processor it sets matters: removing it alone changes the ids), the CPU
restatement (tests/proc_oracle.py) must reproduce them, and every live decision keeps a top-1 vs top-2 margin >= 2e-3 after the
processors (sampler) or passes the beam screens of make_beam_golden.py (>= 1e-3).  Seeds, settings and ids are stored.

    python scripts/make_processor_golden.py        (PROC_FULL=0 skips the full-size case)
"""
import json
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
import make_beam_golden as MBG            # noqa: E402
import proc_oracle as PO                  # noqa: E402

EOS = 1025
REP = 2.0
MARGIN = 2e-3


class _Tap:
    """pass-through processor in front of the warpers: the top-1 / top-2 gap of the processed scores, per row and step"""
    def __init__(self):
        self.gaps = []

    def __call__(self, input_ids, scores):
        t2 = torch.topk(scores, 2, dim=-1)[0]
        self.gaps.append((t2[:, 0] - t2[:, 1]).numpy().copy())
        return scores


def sample_stream(g, SG, cond, codes, kw, max_new, rep=REP):
    """the reference loop with _get_logits_processor's list for (repetition_penalty, top_k=1, do_sample=True, **kw)"""
    from transformers import GenerationConfig, GenerationMixin, LogitsProcessorList
    from transformers.generation.logits_process import TopKLogitsWarper
    from transformers.generation.stopping_criteria import MaxLengthCriteria
    import types as _t
    gi = g.gpt_inference
    gi.generation_config = GenerationConfig()
    gi._update_model_kwargs_for_generation = _t.MethodType(GenerationMixin._update_model_kwargs_for_generation, gi)
    gi._merge_criteria_processor_list = _t.MethodType(GenerationMixin._merge_criteria_processor_list, gi)
    fake = g.compute_embeddings(cond, codes)
    n0 = fake.shape[1]
    cfg = GenerationConfig(do_sample=True, top_k=1, top_p=1.0, temperature=1.0, repetition_penalty=rep, eos_token_id=EOS,
                           pad_token_id=EOS, **kw)
    cfg._eos_token_tensor = torch.tensor([EOS])
    procs = GenerationMixin._get_logits_processor(gi, generation_config=cfg, input_ids_seq_length=n0, encoder_input_ids=fake,
                                                  logits_processor=LogitsProcessorList(), device="cpu")
    tap = _Tap()
    i = next(i for i, p in enumerate(procs) if isinstance(p, TopKLogitsWarper))
    procs.insert(i, tap)
    pairs = SG.NewGenerationMixin.sample_stream(
        gi, fake, logits_processor=procs, logits_warper=LogitsProcessorList(),
        stopping_criteria=MG._StoppingCriteria433([MaxLengthCriteria(max_length=n0 + max_new)]), pad_token_id=EOS, eos_token_id=EOS,
        output_attentions=False, output_hidden_states=True, attention_mask=torch.ones_like(fake), use_cache=True)
    with torch.inference_mode():
        toks = [t for t, _ in pairs]
    return torch.stack(toks, 1).numpy(), np.stack(tap.gaps, 1), [type(p).__name__ for p in procs]


def live_min(toks, gaps):
    m = np.inf
    for b in range(toks.shape[0]):
        hit = np.nonzero(toks[b] == EOS)[0]
        end = int(hit[0]) + 1 if len(hit) else toks.shape[1]
        m = min(m, float(gaps[b, :end].min()))
    return m


def ablation(kw, run, ids):
    """the first kwarg whose removal alone leaves the ids as they are (that kwarg does not matter in this case), else None"""
    for k in kw:
        other = run({j: v for j, v in kw.items() if j != k})
        if other.shape == ids.shape and np.array_equal(other, ids):
            return k
    return None


def sampler_case(GPT, SG, tag, model_args, seed, in_seeds, B, Tc, max_new, make_kw, stop_bias=None, need_ragged=False, rep=REP):
    """make_kw(baseline tokens) -> the processor kwargs; the first input seed whose case passes every screen is kept"""
    dims = gcfg.gpt_dims(model_args)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][EOS] = float(stop_bias)
    g = MG.build_ref_gpt(GPT, model_args, w)
    ora = BO.OracleGpt(w, dims)
    for in_seed in in_seeds:
        cond, codes = MG.gpt_inputs(in_seed, dims, B, Tc)
        base, _, _ = sample_stream(g, SG, cond, codes, {}, max_new, rep)
        kw = make_kw(base)
        toks, gaps, names = sample_stream(g, SG, cond, codes, kw, max_new, rep)
        why = None
        if base.shape == toks.shape and np.array_equal(base, toks):
            why = "processors change nothing"
        elif live_min(toks, gaps) < MARGIN:
            why = f"margin {live_min(toks, gaps):.1e}"
        else:
            ct, _ = PO.greedy(ora, cond, codes, kw, rep, max_new)
            ends = [int(np.argmax(r == EOS)) if (r == EOS).any() else -1 for r in toks]
            if not np.array_equal(ct, toks):
                why = "CPU restatement differs"
            elif need_ragged and (min(ends) < 0 or len(set(ends)) < 2):
                why = f"not ragged {ends}"
            else:
                k = ablation(kw, lambda kk: sample_stream(g, SG, cond, codes, kk, max_new, rep)[0], toks)
                if k is not None:
                    why = f"{k} does not matter"
        if why is None:
            break
        print(f"  {tag}: in_seed {in_seed} rejected ({why})")
    else:
        raise RuntimeError(f"{tag}: no input seed passed the screens")
    print(f"{tag}: in_seed {in_seed} kw {kw} -> {toks.shape}, base {base.shape}, margin {live_min(toks, gaps):.2e}, {names}")
    return {f"{tag}_tokens": toks, f"{tag}_base": base, f"{tag}_margins": gaps, f"{tag}_seed": np.int64(seed),
            f"{tag}_in_seed": np.int64(in_seed), f"{tag}_B": np.int64(B), f"{tag}_Tc": np.int64(Tc), f"{tag}_max_new": np.int64(max_new),
            f"{tag}_stop_bias": np.float64(stop_bias if stop_bias is not None else 0.0), f"{tag}_kw": np.array(json.dumps(kw)),
            f"{tag}_full": np.int64(model_args is gcfg.DEFAULT_MODEL_ARGS), f"{tag}_kind": np.array("sampler"),
            f"{tag}_rep": np.float64(rep)}


def beam_case(GPT, tag, model_args, seed, in_seeds, B, Tc, K, lp, max_new, make_kw, stop_bias=None, rep=REP):
    dims = gcfg.gpt_dims(model_args)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][EOS] = float(stop_bias)
    g = MBG.arm_beam(MG.build_ref_gpt(GPT, model_args, w))
    ora = BO.OracleGpt(w, dims)
    for in_seed in in_seeds:
        cond, codes = MG.gpt_inputs(in_seed, dims, B, Tc)
        base = MBG.ref_beam(g, cond, codes, K, lp, rep, max_new)
        kw = make_kw(base)
        g.max_gen_mel_tokens = max_new

        def run(kk):
            with torch.inference_mode():
                return g.generate(cond, codes, num_beams=K, do_sample=False, length_penalty=lp, repetition_penalty=rep,
                                  num_return_sequences=1, output_attentions=False, **kk).numpy()
        ids = run(kw)
        r = PO.beams(ora, cond, codes, K, lp, rep, max_new, kw)
        why = None
        if base.shape == ids.shape and np.array_equal(base, ids):
            why = "processors change nothing"
        elif r["min_gap"] < 1e-3:
            why = f"gap {r['min_gap']:.1e}"
        elif not np.array_equal(r["ids"], ids):
            why = "CPU restatement differs"
        elif ablation(kw, run, ids) is not None:
            why = f"{ablation(kw, run, ids)} does not matter"
        if why is None:
            break
        print(f"  {tag}: in_seed {in_seed} rejected ({why})")
    else:
        raise RuntimeError(f"{tag}: no input seed passed the screens")
    print(f"{tag}: in_seed {in_seed} kw {kw} -> {ids.shape}, base {base.shape}, gap {r['min_gap']:.2e}")
    return {f"{tag}_tokens": ids, f"{tag}_base": base, f"{tag}_best_scores": r["best_scores"], f"{tag}_min_gap": np.float64(r["min_gap"]),
            f"{tag}_seed": np.int64(seed), f"{tag}_in_seed": np.int64(in_seed), f"{tag}_B": np.int64(B), f"{tag}_Tc": np.int64(Tc),
            f"{tag}_K": np.int64(K), f"{tag}_lp": np.float64(lp), f"{tag}_max_new": np.int64(max_new),
            f"{tag}_stop_bias": np.float64(stop_bias if stop_bias is not None else 0.0), f"{tag}_kw": np.array(json.dumps(kw)),
            f"{tag}_full": np.int64(model_args is gcfg.DEFAULT_MODEL_ARGS), f"{tag}_kind": np.array("beam"), f"{tag}_rep": np.float64(rep)}


def main():
    torch.manual_seed(0)
    GPT, _ = MG.import_reference()
    SG = MG.import_stream_generator()
    tiny = gcfg.TINY_MODEL_ARGS
    out = {}
    cases = []

    def add(d, tag):
        out.update(d)
        cases.append(tag)
    # (a) a stop bias makes EOS come early (ragged over B = 3); min_new_tokens holds it back
    add(sampler_case(GPT, SG, "min_new", tiny, 29, range(4100, 4160), 3, 11, 40, lambda base: dict(min_new_tokens=12),
                     stop_bias=1.2, need_ragged=True), "min_new")
    # (b) min_length (it counts the fake prompt: 46 ids here) holds EOS back, and begin_suppress_tokens bans the first greedy pick
    add(sampler_case(GPT, SG, "min_len_begin", tiny, 29, range(4200, 4300), 3, 11, 40,
                     lambda base: dict(min_length=11 + 32 + 3 + 14, begin_suppress_tokens=[int(base[0, 0])]), stop_bias=1.2,
                     need_ragged=True), "min_len_begin")
    # (c) without a repetition penalty greedy repeats itself: no_repeat_ngram_size bans the repeats (over the whole row, fake
    #     prompt included), and a suppressed token greedy would have picked
    add(sampler_case(GPT, SG, "ngram", tiny, 31, range(4300, 4400), 3, 9, 32,
                     lambda base: dict(no_repeat_ngram_size=2, suppress_tokens=[int(base[1, 3])]), rep=1.0), "ngram")
    add(sampler_case(GPT, SG, "ngram3", tiny, 29, range(4350, 4450), 2, 10, 32, lambda base: dict(no_repeat_ngram_size=3), rep=1.0),
        "ngram3")
    # (d) the EOS decay ends the rows earlier
    add(sampler_case(GPT, SG, "decay", tiny, 29, range(4400, 4460), 3, 11, 40,
                     lambda base: dict(exponential_decay_length_penalty=(4, 1.6)), stop_bias=0.4, need_ragged=True), "decay")
    # beams: min_new_tokens + a stop bias at K = 2; the n-gram ban (no repetition penalty) with a suppressed token at K = 4
    add(beam_case(GPT, "beam_min_new", tiny, 31, range(4500, 4560), 2, 11, 2, 1.0, 24, lambda base: dict(min_new_tokens=10),
                  stop_bias=1.6), "beam_min_new")
    add(beam_case(GPT, "beam_ngram", tiny, 29, range(4600, 4700), 2, 9, 4, 1.0, 24,
                  lambda base: dict(no_repeat_ngram_size=2, suppress_tokens=[int(base[0, 2])]), rep=1.0), "beam_ngram")
    add(beam_case(GPT, "beam_ngram_k2", tiny, 31, range(4700, 4800), 2, 10, 2, 1.0, 24, lambda base: dict(no_repeat_ngram_size=3),
                  rep=1.0), "beam_ngram_k2")
    if os.environ.get("PROC_FULL", "1") == "1":
        add(sampler_case(GPT, SG, "full_ngram", gcfg.DEFAULT_MODEL_ARGS, 3, range(4800, 4830), 1, 12, 40,
                         lambda base: dict(no_repeat_ngram_size=3, suppress_tokens=[int(base[0, 1])]), rep=1.0), "full_ngram")
    out["cases"] = np.array(json.dumps(cases))
    np.savez_compressed(os.path.join(MG.GOLD, "logits_processors.npz"), **out)


if __name__ == "__main__":
    main()
