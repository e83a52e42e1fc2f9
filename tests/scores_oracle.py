"""Test infrastructure: GPT.generate(return_dict_in_generate=True, output_scores=True, output_logits=True) restated on the CPU.  The
model is the oracle's GPT forward (tests/beam_oracle.py: OracleGpt); what follows it is the installed transformers' own processor and
warper objects, EXECUTED, in the order GenerationMixin._get_logits_processor builds them (tests/cfg_oracle.py: hf_chain).  As in
GenerationMixin._sample, `logits[t]` is the raw head output of step t and `scores[t]` what the processor list returns for it; rows
that have stopped are fed the stop token (pad = eos) and keep producing rows.  `gather` is compute_transition_scores without beams,
and `hf_gather` the installed transformers' own method, executed on a stub, to pin it to."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cfg_oracle as CF      # noqa: E402

O = CF.O


@torch.inference_mode()
def decode(ora, cond, codes, rep=1.0, kw=None, max_new=12, sampling=None, forced=None):
    """Unguided decoding on the oracle: greedy (argmax of the scores, first index) unless `forced` [B, n] gives the tokens to feed
    (teacher forcing).  sampling: None (do_sample=False: no warpers, no temperature) or dict(temperature, top_k) (do_sample=True).
    Runs to the step where the last row stops (max_new at most; all of `forced`).
    -> dict(ids [B, n] int64 numpy; logits [n][B, V]; scores [n][B, V]; margins [B, n] numpy: top-1 vs top-2 of the scores, inf once the
    row has stopped)"""
    kw = kw or {}
    eos = ora.dims["stop_audio_token"]
    fake, logits, cache = ora.prefill(cond, codes)
    B, n0 = fake.shape
    chain = CF.hf_chain(kw, n0, eos, rep, sampling)
    ids = fake.long()
    fin = torch.zeros(B, dtype=torch.bool)
    toks, raw, scores, gaps = [], [], [], []
    n = max_new if forced is None else int(forced.shape[1])
    for t in range(n):
        s = logits.float().clone()
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
        raw.append(logits.float().clone())
        scores.append(s)
        gaps.append(gap)
        ids = torch.cat([ids, x[:, None]], 1)
        fin = fin | (x == eos)
        if (forced is None and bool(fin.all())) or t == n - 1:
            break
        logits, cache = ora.step(cache, x, t + 1)
    return dict(ids=torch.stack(toks, 1).numpy(), logits=raw, scores=scores, margins=torch.stack(gaps, 1).numpy())


def gather(scores, tokens, normalize):
    """compute_transition_scores without beams: scores [n][R, V] (or a [R, n, V] tensor), tokens [R, n] -> [R, n] fp32"""
    s = scores if torch.is_tensor(scores) else torch.stack(list(scores), 1)
    s = s.float()
    if normalize:
        # in HF's layout, [R, V, n] reduced over the middle dimension: torch's log_softmax rounds by layout, and this one is pinned bit
        # for bit to the executed method (tests/test_scores_host.py)
        s = torch.log_softmax(s.permute(0, 2, 1).contiguous(), dim=1).permute(0, 2, 1)
    return s.gather(2, tokens.long()[:, :, None]).squeeze(2)


class _Stub:
    """the `self` GenerationMixin.compute_transition_scores reads: a config that carries vocab_size"""

    def __init__(self, vocab):
        cfg = type("C", (), {"vocab_size": vocab})()
        cfg.get_text_config = lambda *a, **k: cfg
        self.config = cfg


def hf_gather(scores, tokens, normalize, vocab):
    """the installed transformers' GenerationMixin.compute_transition_scores, executed: scores a tuple of n [R, V] rows"""
    from transformers import GenerationMixin
    return GenerationMixin.compute_transition_scores(_Stub(vocab), tokens.long(), tuple(scores), normalize_logits=bool(normalize))
