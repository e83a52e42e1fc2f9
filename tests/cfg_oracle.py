"""Test infrastructure: classifier-free guidance (GPT.generate(guidance_scale=s, negative_cond_latents=...)) restated on the CPU.  The
conditional and the unconditional prompt each run the oracle's GPT forward (tests/beam_oracle.py: OracleGpt) and are fed the same
tokens; the combine step is the installed transformers' own UnbatchedClassifierFreeGuidanceLogitsProcessor, EXECUTED, with a stub
`model` that hands it the oracle's unconditional logits; behind it come HF's own processor objects in the order
GenerationMixin._get_logits_processor builds them: [CFG, RepetitionPenalty, the length / repetition processors of
proc_oracle.hf_processors, (sampling) Temperature, TopK].  `closed_form` is the same combine written out, for the test that pins it
to the executed class."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import beam_oracle as BO      # noqa: E402
import proc_oracle as PO      # noqa: E402

O = BO.O


def closed_form(cond, uncond, scale):
    """s * (lsm(cond) - lsm(uncond)) + lsm(uncond) on [B, V] fp32 rows, in HF's operation order"""
    lc = torch.nn.functional.log_softmax(cond.float(), dim=-1)
    lu = torch.nn.functional.log_softmax(uncond.float(), dim=-1)
    return scale * (lc - lu) + lu


class _Out(dict):
    """what the guidance processor reads of a model output: .logits and .get("past_key_values")"""
    logits = None


class _UncondModel:
    """the `model` of UnbatchedClassifierFreeGuidanceLogitsProcessor: returns the unconditional logits row it was last given"""

    def __init__(self):
        self.row = None
        self.calls = 0

    def __call__(self, input_ids, **kwargs):
        self.calls += 1
        out = _Out()
        out.logits = self.row[:, None, :]
        return out


def hf_guidance(scale):
    """(processor, stub): set stub.row = unconditional logits [B, V] before every processor(ids, conditional logits) call"""
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    stub = _UncondModel()
    return UnbatchedClassifierFreeGuidanceLogitsProcessor(scale, stub, use_cache=True), stub


def hf_combine(cond, uncond, scale):
    """the executed HF class on [B, V] rows"""
    proc, stub = hf_guidance(scale)
    stub.row = uncond.float()
    out = proc(torch.zeros(cond.shape[0], 1, dtype=torch.long), cond.float())
    assert stub.calls == 1
    return out


def hf_chain(kw, plen, eos, rep, sampling=None):
    """HF's processors behind the guidance processor: RepetitionPenalty (rep != 1), the processors of `kw`, and with sampling =
    dict(temperature, top_k) the Temperature and TopK warpers"""
    from transformers.generation.logits_process import RepetitionPenaltyLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper
    chain = [RepetitionPenaltyLogitsProcessor(float(rep))] if float(rep) != 1.0 else []
    chain += list(PO.hf_processors({k: v for k, v in kw.items() if k in PO.KEYS}, plen, eos, sampling=sampling is not None))
    if sampling is not None:
        if float(sampling.get("temperature", 1.0)) != 1.0:
            chain.append(TemperatureLogitsWarper(float(sampling["temperature"])))
        if int(sampling.get("top_k", 0)) > 0:
            chain.append(TopKLogitsWarper(int(sampling["top_k"])))
    return chain


@torch.inference_mode()
def guided(ora, cond, codes, neg_cond, neg_codes, scale, rep=1.0, kw=None, max_new=12, sampling=None, forced=None):
    """Guided decoding on the oracle.  cond / codes: the conditional prompts [B, 32, d] / [B, Tc]; neg_cond / neg_codes: the
    unconditional ones (their code length may differ).  Greedy (argmax of the final scores) unless `forced` [B, n] gives the tokens to
    feed (teacher forcing: the scores of every step are still computed).  sampling: dict(temperature, top_k) adds HF's warpers to the
    chain (used with `forced`).
    -> dict(ids [B, n] int64, eos-padded once a row has stopped; latents [B, n, d]: the conditional rows' latents; margins [B, n]:
    top-1 vs top-2 of the final scores, inf once the row has stopped; scores [n][B, V]: the final scores of every step)"""
    kw = kw or {}
    w, dims = ora.w, ora.dims
    eos = dims["stop_audio_token"]
    prefix, fake = O.compute_embeddings(w, dims, cond.float(), codes.long())
    z, lc, cache_c = O.gpt_prefill(w, dims, prefix)
    _, lu, cache_u = ora.prefill(neg_cond, neg_codes)
    B, n0 = fake.shape
    cfg, stub = hf_guidance(scale)
    chain = hf_chain(kw, n0, eos, rep, sampling)
    ids = fake.long()
    fin = torch.zeros(B, dtype=torch.bool)
    toks, lats, gaps, scores = [], [], [], []
    n = max_new if forced is None else int(forced.shape[1])
    for t in range(n):
        stub.row = lu.float()
        s = cfg(ids, lc.float())
        for p in chain:
            s = p(ids, s)
        t2 = torch.topk(s, 2, dim=-1)[0]
        gap = (t2[:, 0] - t2[:, 1]).double()
        gap[fin] = np.inf
        if forced is None:
            x = torch.argmax(s, dim=-1)
            x[fin] = eos
        else:
            x = forced[:, t].long()
        toks.append(x)
        lats.append(z)
        gaps.append(gap)
        scores.append(s)
        ids = torch.cat([ids, x[:, None]], 1)
        fin = fin | (x == eos)
        if (forced is None and bool(fin.all())) or t == n - 1:
            break
        z, lc, cache_c = O.gpt_decode_step(w, dims, cache_c, x, t + 1)
        lu, cache_u = ora.step(cache_u, x, t + 1)
    return dict(ids=torch.stack(toks, 1).numpy(), latents=torch.stack(lats, 1), margins=torch.stack(gaps, 1).numpy(), scores=scores)


@torch.inference_mode()
def unguided(ora, cond, codes, rep=1.0, max_new=12):
    """greedy decoding without guidance (proc_oracle.greedy): ids [B, n]"""
    return PO.greedy(ora, cond, codes, {}, rep, max_new)[0]
