"""Test infrastructure: the presence / frequency / windowed repetition penalties of include/genvc_hip.h (gvc_logits_penalties; DESIGN.md
4.29) restated on the CPU, one row and one step at a time, on top of tests/proc_oracle.py and tests/ras_oracle.py.

Counts of a row at a step: n_gen = len - prompt length (the fake prompt ids never count); w = n_gen when the window is 0, else
min(window, n_gen); c_i = how often id i occurs among the row's last w generated ids; ids outside [0, vocab) are ignored.
For every i with c_i > 0: score_i -= frequency * c_i + presence, in fp32 with the fixed order t = fl(fl(f * float(c_i)) + p),
score = fl(score - t) (torch's elementwise fp32 operations round one by one: nothing is fused).
Place in the chain: SequenceBias -> RepetitionPenalty -> HERE -> n-gram / length / suppress processors -> EOS decay -> Temperature.
window > 0 also narrows the multiplicative repetition penalty to the ids with c_i > 0; with the window off it covers every id of the
row, the fake prompt included, once.  A RAS redraw draws from the row that carries the penalties."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import proc_oracle as PO      # noqa: E402
import ras_oracle as RO       # noqa: E402

MARGIN = RO.MARGIN


def counts(row, plen, window, V):
    """int64 [V]: c_i over the last w generated ids of the row (list of ids, fake prompt first)"""
    n_gen = len(row) - min(max(plen, 0), len(row))
    w = n_gen if not window else min(window, n_gen)
    tail = [t for t in row[len(row) - w:] if 0 <= t < V] if w > 0 else []
    return torch.from_numpy(np.bincount(np.asarray(tail, dtype=np.int64), minlength=V).astype(np.int64))


def penalised(logits, row, plen, rep, pen):
    """raw logits [V] fp32 -> the row behind the repetition penalty and the penalties.  pen: (presence, frequency, window) or None"""
    V = logits.numel()
    s = logits.float().clone()
    p, f, W = pen if pen is not None else (0.0, 0.0, 0)
    on = pen is not None and (p != 0.0 or f != 0.0 or W > 0)
    c = counts(row, plen, W, V) if on else torch.zeros(V, dtype=torch.int64)
    hit = c > 0 if (on and W > 0) else torch.zeros(V, dtype=torch.bool).index_fill_(
        0, torch.tensor(sorted({t for t in row if 0 <= t < V}), dtype=torch.long), True)
    s = torch.where(hit, torch.where(s < 0, s * torch.tensor(rep, dtype=torch.float32), s / torch.tensor(rep, dtype=torch.float32)), s)
    if on:
        t = torch.tensor(f, dtype=torch.float32) * c.to(torch.float32)          # fl(f * float(c))
        t = t + torch.tensor(p, dtype=torch.float32)                             # fl(. + p)
        s = torch.where(c > 0, s - t, s)                                         # fl(score - t)
    return s


def full_row(logits, row, plen, samp, kw, eos, pen, temperature=True):
    """the row ahead of truncation: repetition penalty, penalties, the processors of kw, temperature (greedy search: without)"""
    s = penalised(logits, row, plen, samp["repetition_penalty"], pen)
    s = PO.process(s, row, plen, kw, eos)
    return s / samp["temperature"] if temperature else s


def step(logits, row, plen, samp, kw, pen, key, eos, ras=None, finished=False, full=False):
    """one sampler step of one row, as ras_oracle.step with the penalties in the chain.  -> dict(x, tok, redraw, margin1, margin2, c)"""
    s = full_row(logits, row, plen, samp, kw, eos, pen)
    seed, st, r = key
    if samp["top_k"] == 1:
        x, m1 = int(torch.argmax(s)), float("inf")
    else:
        x, m1 = RO.draw(RO.truncated_row(s, samp, kw), RO.rng_uniform(seed, st, r))
    c = RO.count(row, plen, ras[0], x) if ras and ras[0] > 0 else 0
    out = dict(x=x, tok=x, redraw=False, margin1=m1, margin2=float("inf"), c=c)
    if ras and ras[0] > 0 and c >= ras[1] and x != eos and not finished and not full:
        out["tok"], out["margin2"] = RO.draw(s, RO.rng_uniform(seed ^ RO.SALT, st, r))
        out["redraw"] = True
    if finished or full:
        out["tok"] = eos
    return out
