"""Test infrastructure: deterministic beam search (HF `generate(num_beams=K, do_sample=False)`, reference layers/gpt.py:594-609)
restated on the CPU, on the oracle's GPT forward (oracle/genvc_oracle.py).  One `select_step` is what the device's `k_beam_select`
computes (include/genvc_hip.h: gvc_beam_select); `beam_search` runs the whole loop and its finalisation.

Per step and item:
  s = log_softmax(logits) (fp32); repetition penalty on the log-probs over the ids of the beam's input_ids row, each id once;
  s += running score of the beam; top-2K over the K x V candidates; walk them in rank order: an EOS candidate at rank < K becomes
  a finished hypothesis (score / len ** lp, kept set of at most K with BeamHypotheses.add's worst-score bookkeeping), an EOS
  candidate at rank >= K is skipped, the first K non-EOS candidates become the next beams.  An item is done when its kept set is
  full and its worst kept score >= best / len ** lp.
Two length modes (one integer each for the normalisation and the is-done length), t = tokens generated before the step, n0 = prompt
length (fake ids):
  "4.33"       transformers 4.33 (the reference's pin): hypothesis length = n0 + t (the input_ids row, EOS excluded), is-done
               length n0 + t, best = the best candidate of the step; a running beam added at the end has length n0 + T
  "generated"  the installed transformers: generated lengths t + 1 for both, best = the best running beam after the step; a running
               beam added at the end has length T
The margin screen (`min_gap`) is the smallest gap between the K-th and (K+1)-th non-EOS candidate and between any hypothesis score
and the worst kept score it was compared with, over every step of every item."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import genvc_oracle as O          # noqa: E402

MODES = {"4.33": 0, "generated": 1}


class OracleGpt:
    """the oracle's GPT forward with a per-row KV cache that beam reordering can index"""

    def __init__(self, w, dims):
        self.w = {k: (v if torch.is_tensor(v) else torch.as_tensor(v)).float() for k, v in w.items()}
        self.dims = dims

    def prefill(self, cond, codes):
        prefix, fake = O.compute_embeddings(self.w, self.dims, cond.float(), codes.long())
        _, logits, cache = O.gpt_prefill(self.w, self.dims, prefix)
        return fake, logits, cache

    def step(self, cache, tok, j):
        _, logits, cache = O.gpt_decode_step(self.w, self.dims, cache, tok, j)
        return logits, cache


def norm_len(mode, n0, t):
    """the normalisation / is-done length of a hypothesis finished at step t (t tokens before it)"""
    return n0 + t if MODES[mode] == 0 else t + 1


def log_probs(logits, ids, rep):
    """[R, V] fp32 logits, [R, L] int ids -> penalised log-probs (HF RepetitionPenaltyLogitsProcessor on log_softmax)"""
    s = torch.log_softmax(logits.float(), dim=-1)
    ids = ids.long()
    g = torch.gather(s, 1, ids)
    g = torch.where(g < 0, g * rep, g / rep)
    return s.scatter(1, ids, g)


class Hyps:
    """BeamHypotheses (kept set of at most K finished sequences) of one item"""

    def __init__(self, K):
        self.K, self.items, self.worst, self.min_gap = K, [], 1e9, np.inf

    def add(self, score, toks):
        if len(self.items) >= self.K:
            self.min_gap = min(self.min_gap, abs(score - self.worst))
        if len(self.items) < self.K or score > self.worst:
            self.items.append((score, list(toks)))
            if len(self.items) > self.K:
                order = sorted(range(len(self.items)), key=lambda i: (self.items[i][0], i))
                del self.items[order[0]]
                self.worst = sorted(s for s, _ in self.items)[0]
            else:
                self.worst = min(score, self.worst)


def select_step(s, scores, gen, hyps, done, t, n0, K, V, eos, lp, mode):
    """one step for every item.  s [B*K, V] penalised log-probs, scores [B*K] running sums, gen [B*K][t] generated tokens per
    beam, hyps [B] Hyps, done [B] bools.  Returns (tokens [B*K], parents [B*K] (beam within item), new scores [B*K], new gen,
    min_gap of the step); updates hyps and done in place.  A done item keeps its beams (tokens = eos, parents = identity)."""
    B = len(hyps)
    tok = np.full(B * K, eos, dtype=np.int64)
    par = np.tile(np.arange(K), B)
    new_scores = scores.clone()
    new_gen = [list(g) for g in gen]
    gap = np.inf
    acc = s + scores[:, None]
    for b in range(B):
        if done[b]:
            continue
        flat = acc[b * K:(b + 1) * K].reshape(-1)
        top_v, top_i = torch.topk(flat, 2 * K)
        top_v, top_i = top_v.tolist(), top_i.tolist()
        j = 0
        for r, (v, i) in enumerate(zip(top_v, top_i)):
            p, x = i // V, i % V
            if x == eos:
                if r >= K:
                    continue
                hyps[b].add(v / norm_len(mode, n0, t) ** lp, gen[b * K + p])
            else:
                if j < K:
                    tok[b * K + j], par[b * K + j], new_scores[b * K + j] = x, p, v
                    new_gen[b * K + j] = list(gen[b * K + p]) + [x]
                j += 1
            if j == K:
                break
        # the K-th vs the (K+1)-th non-EOS candidate of the whole flat row
        ne = flat.view(K, V).clone()
        ne[:, eos] = -float("inf")
        kk = torch.topk(ne.reshape(-1), K + 1)[0]
        gap = min(gap, float(kk[K - 1] - kk[K]))
        if len(hyps[b].items) >= K:
            best = top_v[0] if MODES[mode] == 0 else float(new_scores[b * K])
            lim = best / norm_len(mode, n0, t) ** lp
            if hyps[b].worst != lim:      # (equal when the best candidate is the eos hypothesis just kept as the worst: the same
                gap = min(gap, abs(hyps[b].worst - lim))     # division on both sides, an exact and deterministic "done")
            done[b] = hyps[b].worst >= lim
        gap = min(gap, hyps[b].min_gap)
    return torch.from_numpy(tok), torch.from_numpy(par), new_scores, new_gen, gap


def finalize(hyps, done, scores, gen, n0, T, K, eos, lp, mode, max_new):
    """add the running beams of the items not done, pick the best hypothesis per item, pad with eos (= pad) to the longest row + 1
    (at most max_new).  Returns (ids int64 [B, n], best scores [B])"""
    B = len(hyps)
    best = []
    for b in range(B):
        if not done[b]:
            L = n0 + T if MODES[mode] == 0 else T
            for k in range(K):
                hyps[b].add(float(scores[b * K + k]) / L ** lp, gen[b * K + k])
        sc, tk = sorted(hyps[b].items, key=lambda x: x[0])[-1]
        best.append((sc, tk))
    width = min(max(len(tk) for _, tk in best) + 1, max_new)
    out = np.full((B, width), eos, dtype=np.int64)
    for b, (_, tk) in enumerate(best):
        out[b, :len(tk)] = tk[:width]
    return out, np.array([sc for sc, _ in best], dtype=np.float64)


@torch.inference_mode()
def beam_search(ora, cond, codes, K, lp, rep, max_new, mode="4.33"):
    """GPT.generate(num_beams=K, do_sample=False, length_penalty=lp, repetition_penalty=rep) on the oracle -> dict(ids [B, n] int64,
    best_scores [B], min_gap, steps)"""
    dims = ora.dims
    eos, V = dims["stop_audio_token"], dims["num_audio_tokens"]
    fake, logits, cache = ora.prefill(cond, codes)
    B, n0 = fake.shape
    rows = torch.arange(B).repeat_interleave(K)
    ids = fake[rows]
    logits = logits[rows]
    cache = [(k[rows], v[rows]) for k, v in cache]
    scores = torch.zeros(B * K)
    scores.view(B, K)[:, 1:] = -1e9
    gen = [[] for _ in range(B * K)]
    hyps = [Hyps(K) for _ in range(B)]
    done = [False] * B
    gap = np.inf
    t = 0
    while True:
        s = log_probs(logits, ids, rep)
        tok, par, scores, gen, g = select_step(s, scores, gen, hyps, done, t, n0, K, V, eos, lp, mode)
        gap = min(gap, g)
        src = (torch.arange(B).repeat_interleave(K) * K + par).long()
        ids = torch.cat([ids[src], tok[:, None]], 1)
        t += 1
        if all(done) or t >= max_new:
            break
        cache = [(k[src], v[src]) for k, v in cache]
        logits, cache = ora.step(cache, tok, t)
    out, best = finalize(hyps, done, scores, gen, n0, t, K, eos, lp, mode, max_new)
    return dict(ids=out, best_scores=best, min_gap=float(gap), steps=t)
