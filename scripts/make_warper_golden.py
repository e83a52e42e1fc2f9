"""tests/golden/logits_warpers.npz: the typical / epsilon / eta sampling warpers EXECUTED on the reference classes under the installed
transformers.  Every case runs the reference's own `NewGenerationMixin.sample_stream` (layers/stream_generator.py), unmodified, driven
as scripts/make_processor_golden.py drives it, with the processor list the installed `GenerationMixin._get_logits_processor` builds for
a GenerationConfig carrying (do_sample=True, top_k, top_p, temperature, repetition_penalty, **warper kwargs).

The cases sample, yet their ids do not depend on the random draw: input seeds are screened so that at EVERY live step exactly one id
survives the warpers (torch.multinomial then has one choice), with margins on that survivor:
  * typical: its probability is >= typical_p + MARGIN, and the key gap to the next surviving id is >= MARGIN (in the combined case,
    where typical keeps several ids: the mass at or below the threshold, and below it, lies >= MARGIN from typical_p, and the
    threshold's key is >= MARGIN from its neighbours);
  * epsilon / eta: the largest probability of the other ids is below the cutoff by >= MARGIN.
The CPU restatement (tests/warp_oracle.py) must reproduce the ids, and each case's ids must change when its warper kwargs are removed
(that run samples: torch.manual_seed(0) before every reference run keeps the file reproducible).  Typical cases must keep an id that is
not the argmax at some step.  Seeds, settings and ids are stored.

    python scripts/make_warper_golden.py        (WARP_FULL=0 skips the full-size case)
"""
import json
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
import warp_oracle as WO                  # noqa: E402

EOS = 1025
MARGIN = 2e-3
WARPERS = ("TypicalLogitsWarper", "EpsilonLogitsWarper", "EtaLogitsWarper")
HARNESS = dict(top_k=15, top_p=0.85, temperature=0.75, repetition_penalty=10.0)     # the reference harness's sampling settings


class _Count:
    """pass-through processor after the warpers: the number of surviving ids per row and step"""
    def __init__(self):
        self.n = []

    def __call__(self, input_ids, scores):
        self.n.append(torch.isfinite(scores).sum(-1).numpy().copy())
        return scores


def sample_stream(g, SG, cond, codes, samp, kw, max_new):
    """the reference loop with _get_logits_processor's list for (do_sample=True, **samp, **kw) -> (ids [B, n], survivors [B, n],
    the processor names)"""
    from transformers import GenerationConfig, GenerationMixin, LogitsProcessorList
    from transformers.generation.stopping_criteria import MaxLengthCriteria
    import types as _t
    gi = g.gpt_inference
    gi.generation_config = GenerationConfig()
    gi._update_model_kwargs_for_generation = _t.MethodType(GenerationMixin._update_model_kwargs_for_generation, gi)
    gi._merge_criteria_processor_list = _t.MethodType(GenerationMixin._merge_criteria_processor_list, gi)
    fake = g.compute_embeddings(cond, codes)
    n0 = fake.shape[1]
    cfg = GenerationConfig(do_sample=True, eos_token_id=EOS, pad_token_id=EOS, **samp, **kw)
    cfg._eos_token_tensor = torch.tensor([EOS])
    procs = GenerationMixin._get_logits_processor(gi, generation_config=cfg, input_ids_seq_length=n0, encoder_input_ids=fake,
                                                  logits_processor=LogitsProcessorList(), device="cpu")
    count = _Count()
    procs.append(count)
    torch.manual_seed(0)
    pairs = SG.NewGenerationMixin.sample_stream(
        gi, fake, logits_processor=procs, logits_warper=LogitsProcessorList(),
        stopping_criteria=MG._StoppingCriteria433([MaxLengthCriteria(max_length=n0 + max_new)]), pad_token_id=EOS, eos_token_id=EOS,
        output_attentions=False, output_hidden_states=True, attention_mask=torch.ones_like(fake), use_cache=True)
    with torch.inference_mode():
        toks = [t for t, _ in pairs]
    return torch.stack(toks, 1).numpy(), np.stack(count.n, 1), [type(p).__name__ for p in procs]


def live(toks, a):
    """a [B, n, ...] restricted to each row's live steps (up to and including its eos)"""
    out = []
    for b in range(toks.shape[0]):
        hit = np.nonzero(toks[b] == EOS)[0]
        end = int(hit[0]) + 1 if len(hit) else toks.shape[1]
        out.append(a[b, :end])
    return np.concatenate(out, 0)


def case(GPT, SG, tag, model_args, seed, in_seeds, B, Tc, max_new, samp, kw, need_off_argmax=False):
    dims = gcfg.gpt_dims(model_args)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    g = MG.build_ref_gpt(GPT, model_args, w)
    ora = BO.OracleGpt(w, dims)
    for in_seed in in_seeds:
        cond, codes = MG.gpt_inputs(in_seed, dims, B, Tc)
        toks, surv, names = sample_stream(g, SG, cond, codes, samp, kw, max_new)
        why = None
        if not (live(toks, surv) == 1).all():
            why = f"{int((live(toks, surv) > 1).sum())} steps keep several ids"
        else:
            ct, marg, amax = WO.single_survivor(ora, cond, codes, kw, samp, max_new)
            m = live(ct, marg) if ct.shape == toks.shape else None
            if not np.array_equal(ct, toks):
                why = "CPU restatement differs"
            elif not (m[:, 0] == 1).all():
                why = "restatement keeps several ids"
            elif min(m[:, 1].min(), m[:, 2].min(), m[:, 3].min()) < MARGIN:
                why = f"margins {m[:, 1].min():.1e} / {m[:, 2].min():.1e} / {m[:, 3].min():.1e}"
            elif need_off_argmax and not (live(ct, (ct != amax)[..., None])).any():
                why = "the survivor is the argmax at every step"
            else:
                base, _, _ = sample_stream(g, SG, cond, codes, samp, {}, max_new)
                if base.shape == toks.shape and np.array_equal(base, toks):
                    why = "the warpers change nothing"
        if why is None:
            break
        print(f"  {tag}: in_seed {in_seed} rejected ({why})")
    else:
        raise RuntimeError(f"{tag}: no input seed passed the screens")
    off = int(live(ct, (ct != amax)[..., None]).sum())
    print(f"{tag}: in_seed {in_seed} samp {samp} kw {kw} -> {toks.shape}, base {base.shape}, margins {m[:, 1].min():.2e} / "
          f"{m[:, 2].min():.2e} / {m[:, 3].min():.2e}, {off} steps off the argmax, {[n for n in names if n in WARPERS]}")
    return {f"{tag}_tokens": toks, f"{tag}_base": base, f"{tag}_margins": marg, f"{tag}_argmax": amax, f"{tag}_seed": np.int64(seed),
            f"{tag}_in_seed": np.int64(in_seed), f"{tag}_B": np.int64(B), f"{tag}_Tc": np.int64(Tc), f"{tag}_max_new": np.int64(max_new),
            f"{tag}_samp": np.array(json.dumps(samp)), f"{tag}_kw": np.array(json.dumps(kw)),
            f"{tag}_full": np.int64(model_args is gcfg.DEFAULT_MODEL_ARGS)}


def main():
    torch.manual_seed(0)
    GPT, _ = MG.import_reference()
    SG = MG.import_stream_generator()
    tiny = gcfg.TINY_MODEL_ARGS
    # without top_k the synthetic logits are near-flat over 1026 ids (p1 ~ 0.01 at temperature 1): the single-warper cases sharpen them
    plain = dict(top_k=20, top_p=1.0, temperature=0.3, repetition_penalty=2.0)
    out = {}
    cases = []

    def add(d, tag):
        out.update(d)
        cases.append(tag)
    add(case(GPT, SG, "typical", tiny, 29, range(5000, 5200), 2, 11, 20, plain, dict(typical_p=0.05), need_off_argmax=True), "typical")
    add(case(GPT, SG, "epsilon", tiny, 29, range(5200, 5400), 2, 11, 20, plain, dict(epsilon_cutoff=0.25)), "epsilon")
    add(case(GPT, SG, "eta", tiny, 29, range(5400, 5600), 2, 11, 20, dict(plain, top_k=0, temperature=0.05), dict(eta_cutoff=0.95)), "eta")
    # typical keeps several ids (not always the argmax), the cutoffs leave the most probable of them
    add(case(GPT, SG, "harness", tiny, 31, range(5600, 5800), 2, 11, 20, HARNESS,
             dict(typical_p=0.5, epsilon_cutoff=0.3, eta_cutoff=0.3), need_off_argmax=True), "harness")
    if os.environ.get("WARP_FULL", "1") == "1":
        add(case(GPT, SG, "full_typical", gcfg.DEFAULT_MODEL_ARGS, 3, range(5800, 5840), 1, 12, 12, plain, dict(typical_p=0.05),
                 need_off_argmax=True), "full_typical")
    out["cases"] = np.array(json.dumps(cases))
    np.savez_compressed(os.path.join(MG.GOLD, "logits_warpers.npz"), **out)


if __name__ == "__main__":
    main()
