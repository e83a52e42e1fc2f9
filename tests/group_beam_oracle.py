"""Test infrastructure: group (diverse) beam search -- HF `generate(num_beams=K, num_beam_groups=G, diversity_penalty=lam,
do_sample=False)` -- restated on the CPU on top of tests/nbest_oracle.py.  The semantics are transformers 4.33's group_beam_search,
HammingDiversityLogitsProcessor and BeamSearchScorer with num_beam_groups, restated from the published source (the installed
transformers no longer ships the mode, so nothing here is executed HF code; tests/test_group_beam_host.py ties the restatement to the
executed plain searches wherever the semantics allow).  DESIGN.md 4.12; include/genvc_hip.h: gvc_beam_groups.

The K rows of item b are G groups of S = K / G: rows b*K + g*S + i belong to group g.  The running score starts at 0 for the first beam
of every group and at -1e9 for the others.  Per step the groups run in order; for the S rows of group g:
  s = log_softmax(logits) (fp32); for g > 0: s[x] -= lam * f[x], f[x] = how often token x was chosen at this step by the rows of groups
  0..g-1 of the item (a done group counts as eos S times; eos is penalised like any x); the repetition penalty over the ids of the row,
  each id once; the processors (tests/proc_oracle.py), if any; s += running score; then nbest_oracle.select_step with K replaced by S
  on the group's own kept set (capacity S) and done flag.  Parents are beams of the same group.
A done group keeps its beams (tokens = eos, parents = identity); the item is done when all its groups are.  Finalisation: the running
beams of every group not done join that group's set; the N best hypotheses over the G sets of the item are returned best first.
`min_gap` holds every comparison the groups make, `order_gap` the smallest pairwise distance of all kept scores of an item."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402
import nbest_oracle as NO                     # noqa: E402
import proc_oracle as PO                      # noqa: E402


def penalise(s, ids, rep):
    """the repetition penalty of beam_oracle.log_probs on given log-probs s [R, V] (ids [R, L])"""
    ids = ids.long()
    g = torch.gather(s, 1, ids)
    g = torch.where(g < 0, g * rep, g / rep)
    return s.scatter(1, ids, g)


def start_scores(B, K, G):
    sc = torch.full((B, K), -1e9)
    sc[:, ::K // G] = 0.0
    return sc.reshape(-1)


def select_step(ls, ids, scores, gen, hyps, done, t, n0, K, G, lam, V, eos, lp, rep, mode, early_stopping=False, max_new=None,
                proc_kw=None):
    """one step for every item and group.  ls [B*K, V] = log_softmax(logits), ids [B*K, L] the input_ids rows, scores [B*K] running
    sums, gen [B*K][t], hyps [B][G] BO.Hyps(S), done [B][G] bools (both updated in place).  Returns (tokens [B*K], parents [B*K] (beam
    within the item), new scores, new gen, min_gap of the step)"""
    B, S = len(hyps), K // G
    tok = torch.full((B * K,), eos, dtype=torch.int64)
    par = torch.arange(K).repeat(B)
    new_scores = scores.clone()
    new_gen = [list(x) for x in gen]
    freq = torch.zeros(B, V)
    gap = np.inf
    for g in range(G):
        rows = torch.tensor([b * K + g * S + i for b in range(B) for i in range(S)])
        s = ls[rows].clone()
        if g > 0:
            s = s - lam * freq.repeat_interleave(S, 0)
        s = penalise(s, ids[rows], rep)
        if proc_kw:
            s = torch.stack([PO.process(s[r], list(map(int, ids[rows[r]])), n0, proc_kw, eos) for r in range(B * S)])
        hy = [hyps[b][g] for b in range(B)]
        dn = [done[b][g] for b in range(B)]
        tk, pr, sc, gn, gp = NO.select_step(s, scores[rows], [gen[r] for r in rows.tolist()], hy, dn, t, n0, S, V, eos, lp, mode,
                                            early_stopping, max_new)
        gap = min(gap, gp)
        tok[rows], par[rows], new_scores[rows] = tk, pr + g * S, sc
        for j, r in enumerate(rows.tolist()):
            new_gen[r] = gn[j]
            freq[r // K, int(tk[j])] += 1.0
        for b in range(B):
            done[b][g] = dn[b]
    return tok, par, new_scores, new_gen, gap


def finalize(hyps, done, scores, gen, n0, T, K, G, eos, lp, mode, max_new, num_return=1):
    """-> (ids int64 [B*N, n], scores [B*N], order_gap, group of every returned row [B*N])"""
    B, S, N = len(hyps), K // G, num_return
    rows, gap = [], np.inf
    L = n0 + T if BO.MODES[mode] == 0 else T
    for b in range(B):
        cand = []
        for g in range(G):
            if not done[b][g]:
                for k in range(b * K + g * S, b * K + (g + 1) * S):
                    hyps[b][g].add(float(scores[k]) / L ** lp, gen[k])
            cand.extend((sc, tk, g) for sc, tk in hyps[b][g].items)
        kept = sorted(cand, key=lambda x: x[0])[::-1]
        sc = [x[0] for x in kept]
        gap = min([gap] + [sc[i] - sc[i + 1] for i in range(len(sc) - 1)])
        rows.extend(kept[:N])
    width = min(max(len(tk) for _, tk, _ in rows) + 1, max_new)
    out = np.full((B * N, width), eos, dtype=np.int64)
    for r, (_, tk, _) in enumerate(rows):
        out[r, :len(tk)] = tk[:width]
    return out, np.array([sc for sc, _, _ in rows], dtype=np.float64), float(gap), np.array([g for _, _, g in rows], dtype=np.int64)


@torch.inference_mode()
def group_beam_search(ora, cond, codes, K, G, lam, lp, rep, max_new, mode="4.33", early_stopping=False, num_return=1, proc_kw=None):
    """GPT.generate(num_beams=K, num_beam_groups=G, diversity_penalty=lam, do_sample=False, ...) on the oracle -> dict(ids [B*N, n],
    scores [B*N], kept [B][G] sorted (score, tokens) sets after finalisation, row_groups [B*N], min_gap, order_gap, steps,
    staggered: some group was done while another group of its item still ran)"""
    dims = ora.dims
    eos, V = dims["stop_audio_token"], dims["num_audio_tokens"]
    fake, logits, cache = ora.prefill(cond, codes)
    B, n0 = fake.shape
    S = K // G
    rows = torch.arange(B).repeat_interleave(K)
    ids = fake[rows]
    logits = logits[rows]
    cache = [(k[rows], v[rows]) for k, v in cache]
    scores = start_scores(B, K, G)
    gen = [[] for _ in range(B * K)]
    hyps = [[BO.Hyps(S) for _ in range(G)] for _ in range(B)]
    done = [[False] * G for _ in range(B)]
    gap, staggered, t = np.inf, False, 0
    while True:
        ls = torch.log_softmax(logits.float(), dim=-1)
        tok, par, scores, gen, g = select_step(ls, ids, scores, gen, hyps, done, t, n0, K, G, lam, V, eos, lp, rep, mode, early_stopping,
                                               max_new, proc_kw)
        gap = min(gap, g)
        src = (torch.arange(B).repeat_interleave(K) * K + par).long()
        ids = torch.cat([ids[src], tok[:, None]], 1)
        t += 1
        staggered = staggered or any(any(d) and not all(d) for d in done)
        if all(all(d) for d in done) or t >= max_new:
            break
        cache = [(k[src], v[src]) for k, v in cache]
        logits, cache = ora.step(cache, tok, t)
    out, sc, order_gap, row_groups = finalize(hyps, done, scores, gen, n0, t, K, G, eos, lp, mode, max_new, num_return)
    kept = [[sorted((s_, list(tk)) for s_, tk in hyps[b][g].items) for g in range(G)] for b in range(B)]
    return dict(ids=out, scores=sc, kept=kept, row_groups=row_groups, min_gap=float(gap), order_gap=order_gap, steps=t,
                staggered=staggered)
