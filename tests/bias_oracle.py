"""Test infrastructure: sequence_bias, bad_words_ids, forced_eos_token_id, forced_bos_token_id and renormalize_logits of GPT.generate
(include/genvc_hip.h: gvc_logits_bias) on the CPU.  The oracle is the installed transformers' own classes, EXECUTED:
SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor, ForcedBOSTokenLogitsProcessor, ForcedEOSTokenLogitsProcessor and
LogitNormalization, in the places GenerationMixin._get_logits_processor gives them among the processors of tests/proc_oracle.py
(hf_processors) and the warpers of tests/cfg_oracle.py (hf_chain):
  [guidance] -> SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> MinLength -> MinNewTokens -> ForcedBOS -> ForcedEOS ->
  ExponentialDecay -> Suppress -> SuppressAtBegin -> [sampling: Temperature, TopK] -> LogitNormalization.
`process` restates the same chain one row at a time, as the device applies it, and tests/test_bias_host.py pins it to the executed
chain; `decode` runs the chain on the oracle's GPT forward (tests/beam_oracle.py: OracleGpt), unguided or behind the executed guidance
processor of tests/cfg_oracle.py."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import cfg_oracle as CF      # noqa: E402
import proc_oracle as PO     # noqa: E402

KEYS = ("sequence_bias", "bad_words_ids", "forced_eos_token_id", "forced_bos_token_id", "renormalize_logits")
NINF = -float("inf")

# the class names of the executed chain with every kwarg on, in order (tests/test_bias_host.py asserts it)
ORDER = ["SequenceBiasLogitsProcessor", "RepetitionPenaltyLogitsProcessor", "NoRepeatNGramLogitsProcessor", "NoBadWordsLogitsProcessor",
         "MinLengthLogitsProcessor", "MinNewTokensLengthLogitsProcessor", "ForcedBOSTokenLogitsProcessor",
         "ForcedEOSTokenLogitsProcessor", "ExponentialDecayLengthPenalty", "SuppressTokensLogitsProcessor",
         "SuppressTokensAtBeginLogitsProcessor", "TemperatureLogitsWarper", "TopKLogitsWarper", "LogitNormalization"]


def hf_chain(kw, plen, eos, rep, max_new, sampling=None):
    """the installed transformers' processor objects for these kwargs, in the order _get_logits_processor builds them.  kw: the
    processor kwargs of proc_oracle.KEYS and the bias kwargs of KEYS; max_new: the call's max_new_tokens (ForcedEOS's max_length is
    plen + max_new); sampling: None (do_sample=False) or dict(temperature, top_k).  LogitNormalization goes last, behind the warpers."""
    from transformers.generation.logits_process import LogitNormalization, TemperatureLogitsWarper, TopKLogitsWarper
    sub = {k: v for k, v in kw.items() if (k in PO.KEYS or k in KEYS) and k != "renormalize_logits" and v is not None}
    if float(rep) != 1.0:
        sub["repetition_penalty"] = float(rep)
    sub["max_length"] = int(plen) + int(max_new)
    chain = list(PO.hf_processors(sub, plen, eos, sampling=sampling is not None))
    if sampling is not None:
        if float(sampling.get("temperature", 1.0)) != 1.0:
            chain.append(TemperatureLogitsWarper(float(sampling["temperature"])))
        if int(sampling.get("top_k", 0)) > 0:
            chain.append(TopKLogitsWarper(int(sampling["top_k"])))
    if kw.get("renormalize_logits"):
        chain.append(LogitNormalization())
    return chain


def run_chain(chain, ids, scores):
    s = scores.float().clone()
    for p in chain:
        s = p(ids, s)
    return s


def entries(kw, eos):
    """(sequence_bias entries in the order of application: length-1 first, then dict order; bad-word entries without a bare [eos])"""
    sb = kw.get("sequence_bias") or {}
    if not isinstance(sb, dict):
        sb = {tuple(e[0]): e[1] for e in sb}
    seqs = [(tuple(k), float(v)) for k, v in sb.items() if len(k) == 1] + [(tuple(k), float(v)) for k, v in sb.items() if len(k) > 1]
    bans = [tuple(b) for b in (kw.get("bad_words_ids") or []) if list(b) != [eos]]
    return seqs, bans


def hits(row, seq):
    m = len(seq)
    return m == 1 or (m <= len(row) and list(row[len(row) - (m - 1):]) == list(seq[:-1]))


def process(logits, row, plen, kw, eos, rep=1.0, max_new=None):
    """logits [V] fp32: the raw (or guided) row; row: the input_ids row (list); plen: its prompt length -> the processed scores of a
    greedy search (no warpers), as the device computes them: the bias accumulates from 0 in fp32, one add per hit entry, and is added
    to the logit once, ahead of the repetition penalty; bans and the forced EOS are -inf writes at their places in the order"""
    s = logits.float().clone()
    L = len(row)
    seqs, bans = entries(kw, eos)
    if seqs:
        bias = torch.zeros_like(s)
        for seq, v in seqs:
            if hits(row, seq):
                bias[seq[-1]] = bias[seq[-1]] + torch.tensor(v, dtype=torch.float32)
        s = s + bias
    if float(rep) != 1.0:
        s = PO.rep_penalty(s, row, float(rep))
    for x in PO.ngram_bans(row, kw.get("no_repeat_ngram_size") or 0):
        s[x] = NINF
    for seq in bans:
        if hits(row, seq):
            s[seq[-1]] = NINF
    if (kw.get("min_length") or 0) > 0 and L < kw["min_length"]:
        s[eos] = NINF
    if (kw.get("min_new_tokens") or 0) > 0 and L - plen < kw["min_new_tokens"]:
        s[eos] = NINF
    # (ForcedBOS fires at L == 1: never, the prompt is longer)
    if kw.get("forced_eos_token_id") is not None and L == plen + max_new - 1:
        s = torch.full_like(s, NINF)
        s[eos] = 0.0
    rest = {k: kw.get(k) for k in ("exponential_decay_length_penalty", "suppress_tokens", "begin_suppress_tokens")}
    s = PO.process(s, row, plen, rest, eos)
    if kw.get("renormalize_logits"):
        s = torch.log_softmax(s, -1)
    return s


@torch.inference_mode()
def decode(ora, cond, codes, rep=1.0, kw=None, max_new=12, sampling=None, forced=None, guide=None):
    """scores_oracle.decode (guide None) or cfg_oracle.guided (guide = (negative cond, negative codes, scale)) with the chain above.
    Greedy (argmax of the scores, first index) unless `forced` [B, n] gives the tokens to feed.  max_new is the call's max_new_tokens
    whatever the length of `forced`.
    -> dict(ids [B, n] int64 numpy; logits [n][B, V] (the conditional rows); scores [n][B, V]; margins [B, n] numpy)"""
    kw = kw or {}
    eos = ora.dims["stop_audio_token"]
    fake, logits, cache = ora.prefill(cond, codes)
    B, n0 = fake.shape
    chain = hf_chain(kw, n0, eos, rep, max_new, sampling)
    cfg = stub = None
    if guide is not None:
        _, lu, cache_u = ora.prefill(guide[0], guide[1])
        cfg, stub = CF.hf_guidance(guide[2])
    ids = fake.long()
    fin = torch.zeros(B, dtype=torch.bool)
    toks, raw, scores, gaps = [], [], [], []
    n = max_new if forced is None else int(forced.shape[1])
    for t in range(n):
        s = logits.float().clone()
        if cfg is not None:
            stub.row = lu.float()
            s = cfg(ids, s)
        s = run_chain(chain, ids, s)
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
        if cfg is not None:
            lu, cache_u = ora.step(cache_u, x, t + 1)
    return dict(ids=torch.stack(toks, 1).numpy(), logits=raw, scores=scores, margins=torch.stack(gaps, 1).numpy(), n0=n0)
