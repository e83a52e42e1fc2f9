"""Test infrastructure: the length / repetition logits processors of include/genvc_hip.h (gvc_logits_processors) restated on the CPU,
one row at a time, in the order the device applies them (HF _get_logits_processor's):
  repetition penalty -> no_repeat_ngram_size -> min_length -> min_new_tokens -> exponential_decay_length_penalty -> suppress_tokens ->
  begin_suppress_tokens -> [sampling: temperature -> top_k -> top_p] -> min_p.
Lengths are input_ids lengths (the fake prompt of compute_embeddings included); `plen` is the row's prompt length.  `greedy` runs the
sampler loop at top_k = 1 on the oracle's GPT forward, `beams` the beam loop of tests/beam_oracle.py with the processors on each beam's
penalised log-probs."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import beam_oracle as BO      # noqa: E402

KEYS = ("no_repeat_ngram_size", "min_length", "min_new_tokens", "exponential_decay_length_penalty", "suppress_tokens",
        "begin_suppress_tokens", "min_p")


def ngram_bans(row, n):
    """NoRepeatNGram for one row (list of ids): the ids that would complete an n-gram already in the row"""
    L = len(row)
    if not n or L < n:
        return set()
    suf = row[L - n + 1:] if n > 1 else []
    return {row[j + n - 1] for j in range(L - n + 1) if row[j:j + n - 1] == suf}


def rep_penalty(s, row, rep):
    s = s.clone()
    ids = torch.tensor(sorted(set(row)), dtype=torch.long)
    g = s[ids]
    s[ids] = torch.where(g < 0, g * rep, g / rep)
    return s


def process(s, row, plen, kw, eos):
    """s [V] fp32 scores after the repetition penalty, row = the input_ids row (list), plen = its prompt length -> processed scores"""
    s = s.clone()
    L = len(row)
    n = kw.get("no_repeat_ngram_size") or 0
    for x in ngram_bans(row, n):
        s[x] = -float("inf")
    if (kw.get("min_length") or 0) > 0 and L < kw["min_length"]:
        s[eos] = -float("inf")
    if (kw.get("min_new_tokens") or 0) > 0 and L - plen < kw["min_new_tokens"]:
        s[eos] = -float("inf")
    dec = kw.get("exponential_decay_length_penalty")
    if dec is not None:
        idx = L - (dec[0] + plen)
        if idx > 0 and s[eos] > -float("inf"):
            c = torch.tensor(float(dec[1]) ** idx - 1.0, dtype=torch.float32)
            s[eos] = s[eos] + torch.abs(s[eos]) * c
    for x in kw.get("suppress_tokens") or ():
        s[x] = -float("inf")
    if L == plen:
        for x in kw.get("begin_suppress_tokens") or ():
            s[x] = -float("inf")
    return s


def min_p_keep(s, min_p):
    """MinP on scores s [V] (after temperature / top-k / top-p): the kept mask (min_tokens_to_keep = 1)"""
    p = torch.softmax(s, -1)
    keep = ~(p < min_p * p.max())
    keep[int(torch.argmax(p))] = True
    return keep


def hf_processors(kw, plen, eos, sampling=False, num_beams=1):
    """the installed transformers' processor list for these kwargs (GenerationMixin._get_logits_processor), without the repetition
    penalty and the warpers other than min_p"""
    from transformers import GenerationConfig, GenerationMixin
    cfg = GenerationConfig(eos_token_id=eos, pad_token_id=eos, do_sample=sampling, num_beams=num_beams, top_k=None, top_p=None,
                           temperature=None, **{k: v for k, v in kw.items() if v is not None})
    cfg._eos_token_tensor = torch.tensor([eos])

    class _M:
        config = type("C", (), {"is_encoder_decoder": False})()
        _merge_criteria_processor_list = GenerationMixin._merge_criteria_processor_list
    return GenerationMixin._get_logits_processor(_M(), generation_config=cfg, input_ids_seq_length=plen,
                                                 encoder_input_ids=None, logits_processor=None, device="cpu")


@torch.inference_mode()
def greedy(ora, cond, codes, kw, rep, max_new):
    """top_k = 1 decoding (the sampler loop) with the processors: -> (tokens [B, n] int64 padded with eos after a row stops, margins
    [B, n]: top-1 vs top-2 of the processed scores, inf once the row has stopped)"""
    dims = ora.dims
    eos = dims["stop_audio_token"]
    fake, logits, cache = ora.prefill(cond, codes)
    B, n0 = fake.shape
    rows = [list(map(int, r)) for r in fake]
    fin = [False] * B
    toks, gaps = [], []
    for t in range(max_new):
        tok, gap = [], []
        for b in range(B):
            s = process(rep_penalty(logits[b].float(), rows[b], rep), rows[b], n0, kw, eos)
            t2 = torch.topk(s, 2)[0]
            x = int(torch.argmax(s))
            gap.append(float(t2[0] - t2[1]) if not fin[b] else np.inf)
            if fin[b]:
                x = eos
            tok.append(x)
            rows[b].append(x)
            fin[b] = fin[b] or x == eos
        toks.append(tok)
        gaps.append(gap)
        if all(fin):
            break
        logits, cache = ora.step(cache, torch.tensor(tok), t + 1)
    return np.array(toks, dtype=np.int64).T, np.array(gaps).T


@torch.inference_mode()
def beams(ora, cond, codes, K, lp, rep, max_new, kw, mode="generated"):
    """beam_oracle.beam_search with the processors on each beam's penalised log-probs (before the running score)"""
    dims = ora.dims
    eos, V = dims["stop_audio_token"], dims["num_audio_tokens"]
    fake, logits, cache = ora.prefill(cond, codes)
    B, n0 = fake.shape
    src0 = torch.arange(B).repeat_interleave(K)
    ids = fake[src0]
    logits = logits[src0]
    cache = [(k[src0], v[src0]) for k, v in cache]
    scores = torch.zeros(B * K)
    scores.view(B, K)[:, 1:] = -1e9
    gen = [[] for _ in range(B * K)]
    hyps = [BO.Hyps(K) for _ in range(B)]
    done = [False] * B
    gap = np.inf
    t = 0
    while True:
        s = BO.log_probs(logits, ids, rep)
        s = torch.stack([process(s[r], list(map(int, ids[r])), n0, kw, eos) for r in range(B * K)])
        tok, par, scores, gen, g = BO.select_step(s, scores, gen, hyps, done, t, n0, K, V, eos, lp, mode)
        gap = min(gap, g)
        src = (torch.arange(B).repeat_interleave(K) * K + par).long()
        ids = torch.cat([ids[src], tok[:, None]], 1)
        t += 1
        if all(done) or t >= max_new:
            break
        cache = [(k[src], v[src]) for k, v in cache]
        logits, cache = ora.step(cache, tok, t)
    out, best = BO.finalize(hyps, done, scores, gen, n0, t, K, eos, lp, mode, max_new)
    return dict(ids=out, best_scores=best, min_gap=float(gap), steps=t)
