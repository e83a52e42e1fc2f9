"""Test infrastructure: N-best beam search and the three early_stopping modes, restated on top of tests/beam_oracle.py.

early_stopping decides when an item is done, once its kept set holds K hypotheses (t = tokens generated before the step, n0 = prompt
length, max_new = the generation budget):
  False    worst kept score >= best / len ** lp, len = n0 + t ("4.33") or t + 1 ("generated")        (tests/beam_oracle.py)
  True     done at once.  4.33: BeamHypotheses.is_done returns True for a full set.  Installed _beam_search: a full set takes no
           further hypothesis (beams_in_batch_are_full), which is all "done" means for an item
  "never"  as False with len = the longest possible length when lp > 0: max_length = n0 + max_new in 4.33's BeamHypotheses.is_done,
           max_length - decoder_prompt_len = max_new in the installed _check_early_stop_heuristic; lp <= 0: as False
`best` is the best candidate of the step ("4.33") or the best running beam after it ("generated"), as in tests/beam_oracle.py.

Finalisation for num_return_sequences = N (BeamSearchScorer.finalize of 4.33; the installed _beam_search keeps its set sorted and
returns its first N): the running beams of the items not done join their sets, the N best hypotheses per item are returned best first
at rows b*N + j, padded with eos to the longest returned row + 1 (at most max_new).  `order_gap` is the smallest pairwise distance of the
kept scores of an item: the N-best order is unambiguous when it is well above fp32 noise."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402

EARLY = [False, True, "never"]                # the fixture stores the index
TAGS = ["a0", "a1", "a2", "b0", "b1", "c"]   # the cases of tests/golden/nbest.npz (scripts/make_nbest_golden.py)


def done_length(mode, early_stopping, lp, n0, t, max_new):
    """the length the item-done test normalises the best attainable score by"""
    if early_stopping == "never" and lp > 0.0:
        return n0 + max_new if BO.MODES[mode] == 0 else max_new
    return BO.norm_len(mode, n0, t)


def select_step(s, scores, gen, hyps, done, t, n0, K, V, eos, lp, mode, early_stopping=False, max_new=None):
    """beam_oracle.select_step (same arguments, results and walk) with the item-done test of `early_stopping`; the returned gap
    holds the comparisons this mode makes (early_stopping=True compares nothing to decide that an item is done)"""
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
                hyps[b].add(v / BO.norm_len(mode, n0, t) ** lp, gen[b * K + p])
            else:
                if j < K:
                    tok[b * K + j], par[b * K + j], new_scores[b * K + j] = x, p, v
                    new_gen[b * K + j] = list(gen[b * K + p]) + [x]
                j += 1
            if j == K:
                break
        ne = flat.view(K, V).clone()
        ne[:, eos] = -float("inf")
        kk = torch.topk(ne.reshape(-1), K + 1)[0]
        gap = min(gap, float(kk[K - 1] - kk[K]))
        if len(hyps[b].items) >= K:
            if early_stopping is True:
                done[b] = True
            else:
                best = top_v[0] if BO.MODES[mode] == 0 else float(new_scores[b * K])
                lim = best / done_length(mode, early_stopping, lp, n0, t, max_new) ** lp
                if hyps[b].worst != lim:
                    gap = min(gap, abs(hyps[b].worst - lim))
                done[b] = hyps[b].worst >= lim
        gap = min(gap, hyps[b].min_gap)
    return torch.from_numpy(tok), torch.from_numpy(par), new_scores, new_gen, gap


def finalize(hyps, done, scores, gen, n0, T, K, eos, lp, mode, max_new, num_return=1):
    """-> (ids int64 [B*N, n], scores [B*N], order_gap)"""
    B, N = len(hyps), num_return
    rows, gap = [], np.inf
    for b in range(B):
        if not done[b]:
            L = n0 + T if BO.MODES[mode] == 0 else T
            for k in range(K):
                hyps[b].add(float(scores[b * K + k]) / L ** lp, gen[b * K + k])
        kept = sorted(hyps[b].items, key=lambda x: x[0])[::-1]
        sc = [x[0] for x in kept]
        gap = min([gap] + [sc[i] - sc[i + 1] for i in range(len(sc) - 1)])
        rows.extend(kept[:N])
    width = min(max(len(tk) for _, tk in rows) + 1, max_new)
    out = np.full((B * N, width), eos, dtype=np.int64)
    for r, (_, tk) in enumerate(rows):
        out[r, :len(tk)] = tk[:width]
    return out, np.array([sc for sc, _ in rows], dtype=np.float64), float(gap)


@torch.inference_mode()
def beam_search(ora, cond, codes, K, lp, rep, max_new, mode="4.33", early_stopping=False, num_return=1):
    """GPT.generate(num_beams=K, do_sample=False, num_return_sequences=N, early_stopping=...) on the oracle -> dict(ids [B*N, n],
    scores [B*N], min_gap, order_gap, steps)"""
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
    hyps = [BO.Hyps(K) for _ in range(B)]
    done = [False] * B
    gap = np.inf
    t = 0
    while True:
        s = BO.log_probs(logits, ids, rep)
        tok, par, scores, gen, g = select_step(s, scores, gen, hyps, done, t, n0, K, V, eos, lp, mode, early_stopping, max_new)
        gap = min(gap, g)
        src = (torch.arange(B).repeat_interleave(K) * K + par).long()
        ids = torch.cat([ids[src], tok[:, None]], 1)
        t += 1
        if all(done) or t >= max_new:
            break
        cache = [(k[src], v[src]) for k, v in cache]
        logits, cache = ora.step(cache, tok, t)
    out, sc, order_gap = finalize(hyps, done, scores, gen, n0, t, K, eos, lp, mode, max_new, num_return)
    return dict(ids=out, scores=sc, min_gap=float(gap), order_gap=order_gap, steps=t)
