"""Test infrastructure: contrastive search (HF `generate(top_k=K, do_sample=False, penalty_alpha=a)` under transformers 4.33,
reference layers/gpt.py:594-609) restated on the CPU, on the oracle's GPT forward (oracle/genvc_oracle.py).  `rank` is what the device's
similarity + select kernels compute for one step (include/genvc_hip.h: gvc_contrastive_state); `search` runs the whole loop.

Per step and item: s = processors(ids row, logits) (repetition penalty on the raw logits, then the length processors:
tests/proc_oracle.py); p = softmax(s) in fp32; (p_k, x_k) = topk(p, K); each candidate runs one decode step from the item's cache at mel
position t + 1; h_k = ln_f of its row; pen_k = max_j cos(ctx_j, h_k) over the item's context rows (ln_f of every prompt row, then of every
chosen candidate); score_k = (1 - a) p_k - a pen_k; k* = the first argmax.  The token is x_{k*}, or eos once the item has finished.
Margin screens, over every live step: `prob_gap` = the smallest gap between the K-th and (K+1)-th processed score, `score_gap` = the
smallest gap between the best and the second contrastive score; `off_top1` = some step chose a candidate other than the most probable."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import genvc_oracle as O          # noqa: E402
import proc_oracle as PO                      # noqa: E402


def rank(ctx, h, pk, alpha):
    """ctx [B, n, d] context rows, h [B, K, d] candidate rows, pk [B, K] candidate probabilities -> (k* [B], scores [B, K]): HF
    _ranking_fast (each vector normalised, then the dot products; the max over the context; first argmax)"""
    cn = ctx / ctx.norm(dim=2, keepdim=True)
    hn = h / h.norm(dim=2, keepdim=True)
    pen = torch.einsum("bnd,bkd->bkn", cn, hn).max(-1).values
    score = (1.0 - alpha) * pk - alpha * pen
    return score.max(-1).indices, score


@torch.inference_mode()
def prefill(w, dims, cond, codes):
    """-> (fake ids [B, n0], ln_f of every prompt row [B, n0, d], last-row logits [B, V], cache)"""
    prefix, fake = O.compute_embeddings(w, dims, cond.float(), codes.long())
    B = prefix.shape[0]
    row = w["mel_embedding.weight"][dims["start_audio_token"]] + w["mel_pos_embedding.emb.weight"][0]
    emb = torch.cat([prefix, row.view(1, 1, -1).expand(B, 1, -1)], dim=1)
    h, cache = O.gpt_blocks(w, dims, emb)
    _, logits = O.head(w, h[:, -1])
    return fake, h, logits, cache


def process_rows(logits, rows, n0, rep, kw, eos):
    return torch.stack([PO.process(PO.rep_penalty(logits[b].float(), rows[b], rep), rows[b], n0, kw or {}, eos)
                        for b in range(len(rows))])


@torch.inference_mode()
def search(w, dims, cond, codes, K, alpha, rep, max_new, kw=None):
    """the whole loop -> dict(ids int64 [B, n] (eos-padded, n = steps run: the loop stops when every item has finished), lats [B, n, d]
    (the chosen candidates' final_norm latents), prob_gap, score_gap, off_top1, steps)"""
    w = {k: (v if torch.is_tensor(v) else torch.as_tensor(v)).float() for k, v in w.items()}
    eos = dims["stop_audio_token"]
    fake, ctx, logits, cache = prefill(w, dims, cond, codes)
    B, n0 = fake.shape
    d = ctx.shape[-1]
    rows = [list(map(int, r)) for r in fake]
    fin = [False] * B
    cache = [(k.repeat_interleave(K, 0), v.repeat_interleave(K, 0)) for k, v in cache]
    toks, lats = [], []
    prob_gap = score_gap = np.inf
    off_top1 = False
    ar = torch.arange(B)
    for t in range(max_new):
        s = process_rows(logits, rows, n0, rep, kw, eos)
        p = torch.softmax(s, -1)
        pk, tk = torch.topk(p, K, dim=-1)
        emb = (w["mel_embedding.weight"][tk.reshape(-1)] + w["mel_pos_embedding.emb.weight"][t + 1]).unsqueeze(1)
        h, new_cache = O.gpt_blocks(w, dims, emb, cache)
        h = h[:, -1]
        z, lg = O.head(w, h)
        sel, score = rank(ctx, h.view(B, K, d), pk, alpha)
        for b in range(B):
            if fin[b]:
                continue
            sv = torch.topk(s[b], K + 1).values
            prob_gap = min(prob_gap, float(sv[K - 1] - sv[K]))
            sc = torch.sort(score[b], descending=True).values
            score_gap = min(score_gap, float(sc[0] - sc[1]))
            off_top1 = off_top1 or int(sel[b]) != 0
        tok = [eos if fin[b] else int(tk[b, sel[b]]) for b in range(B)]
        for b in range(B):
            rows[b].append(tok[b])
            fin[b] = fin[b] or tok[b] == eos
        toks.append(tok)
        lats.append(z.view(B, K, d)[ar, sel])
        ctx = torch.cat([ctx, h.view(B, K, d)[ar, sel].unsqueeze(1)], 1)
        logits = lg.view(B, K, -1)[ar, sel]
        idx = (ar * K + sel).repeat_interleave(K)
        cache = [(k[idx], v[idx]) for k, v in new_cache]
        if all(fin):
            break
    return dict(ids=np.array(toks, dtype=np.int64).T, lats=torch.stack(lats, 1), prob_gap=prob_gap, score_gap=score_gap,
                off_top1=off_top1, steps=len(toks))


def hidden_rows(w, dims, cond, codes):
    """ln_f of every prompt row [B, n0, d] (what gvc_gpt_prefill_hidden writes)"""
    w = {k: (v if torch.is_tensor(v) else torch.as_tensor(v)).float() for k, v in w.items()}
    return prefill(w, dims, cond, codes)[1]
