"""Test infrastructure: repetition-aware sampling of include/genvc_hip.h (gvc_logits_ras) restated on the CPU, one row and
one step at a time, on top of tests/proc_oracle.py, tests/warp_oracle.py and oracle.genvc_oracle.rng_uniform.  The chain is the sampler's:
  repetition penalty -> processors -> temperature  = the FULL row   -> top_k -> top_p -> min_p -> typical / epsilon / eta = the TRUNCATED row
The first draw takes x from the truncated row with u1 = rng_uniform(seed, step, row).  c = how many of the row's last min(K, n_gen)
generated ids equal x (n_gen = len - prompt length: the fake prompt ids never count).  When c >= min_count, x is not the stop token, the
row is not finished and its ids buffer is not full, x is thrown away and drawn again from the full row with
u2 = rng_uniform(seed ^ SALT, step, row).  Masses run in float64 in vocabulary order; a draw is the first kept index whose running mass
reaches u * total, else the last kept index.  The MARGIN of a draw is the distance in probability between u and the nearer edge of the
bucket it chose: the device's fp32 expf moves an edge by about 1e-7, so a draw whose margin is far above that is the device's draw."""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import proc_oracle as PO      # noqa: E402
import warp_oracle as WO      # noqa: E402
from oracle.genvc_oracle import rng_uniform      # noqa: E402

SALT = 0x5241535F52454452      # GVC_RAS_SALT
NEG = -float("inf")
MARGIN = 1e-5                  # the screen of the GPU tests: about 50 x the edge movement of fp32 expf on a cumulative mass


def min_count(K, tau=0.1):
    """the host's integer threshold: max(1, ceil(tau * K - 1e-9))"""
    return max(1, math.ceil(tau * K - 1e-9))


def full_row(logits, row, plen, samp, kw, eos):
    """raw logits [V] of a row, its input ids (list, fake prompt included) and prompt length -> the row ahead of truncation (fp32):
    repetition penalty, the processors of kw (PO.KEYS without min_p), temperature"""
    s = PO.rep_penalty(logits.float(), row, samp["repetition_penalty"])
    s = PO.process(s, row, plen, kw, eos)
    return s / samp["temperature"]


def truncated_row(s, samp, kw, sampling=True):
    """the full row -> the row the first draw is taken from: top_k (ties with the k-th kept), top_p, min_p, the warpers"""
    k = samp["top_k"]
    x = s.clone()
    if k == 1:
        keep = torch.zeros_like(x, dtype=torch.bool)
        keep[int(torch.argmax(x))] = True          # (first index on ties, as the device's argmax)
        return torch.where(keep, x, torch.full_like(x, NEG))
    if k and 0 < k < x.numel():
        kth = torch.topk(x, k)[0][-1]
        x = x.masked_fill(x < kth, NEG)
    if samp["top_p"] < 1.0 and int(torch.isfinite(x).sum()) > 1:
        sl, si = torch.sort(x, descending=False)
        rem = sl.softmax(-1).cumsum(-1) <= (1 - samp["top_p"])
        rem[-1] = False
        x = x.masked_fill(torch.zeros_like(rem).scatter(0, si, rem), NEG)
    mp = kw.get("min_p") or 0.0
    if mp > 0.0 and sampling:
        x = torch.where(PO.min_p_keep(x, mp), x, torch.full_like(x, NEG))
    return WO.warp(x, kw) if sampling else x


def draw(s, u):
    """inverse-CDF draw on scores s [V] (dropped ids -inf) at the uniform u -> (token, margin).  Weights exp(s - max) in fp32 widened,
    running mass in float64 in vocabulary order"""
    kept = torch.isfinite(s)
    if not bool(kept.any()):
        return 0, 0.0
    e = torch.where(kept, torch.exp(s - s[kept].max()), torch.zeros_like(s)).double().numpy()
    cdf = np.cumsum(e)
    total = float(cdf[-1])
    target = float(np.float32(u)) * total
    hit = np.nonzero((cdf >= target) & kept.numpy())[0]
    if len(hit) == 0:
        return int(np.nonzero(kept.numpy())[0][-1]), 0.0
    t = int(hit[0])
    lo, hi = (cdf[t] - e[t]) / total, cdf[t] / total
    return t, float(min(float(np.float32(u)) - lo, hi - float(np.float32(u))))


def count(row, plen, K, x):
    """c: occurrences of x among the last min(K, n_gen) generated ids of the row"""
    n_gen = len(row) - plen
    w = min(K, n_gen)
    return 0 if w <= 0 else sum(1 for t in row[len(row) - w:] if t == x)


def step(logits, row, plen, samp, kw, ras, key, eos, finished=False, full=False):
    """one sampler step of one row.  logits [V] fp32; row: its input ids (list); samp: repetition_penalty / temperature / top_k /
    top_p; kw: processor and warper kwargs; ras: (window, min_count) or None; key: (seed, step, row) of the first draw; finished /
    full: the row has stopped / its ids buffer is full (the device then emits the stop token)
    -> dict(x: the first draw, tok: what the step emits, redraw, margin1, margin2 (inf when there is no second draw; margin1 is inf
    at top_k = 1, where x is the argmax and nothing is drawn), c)"""
    s = full_row(logits, row, plen, samp, kw, eos)
    seed, st, r = key
    if samp["top_k"] == 1:
        x, m1 = int(torch.argmax(s)), float("inf")
    else:
        x, m1 = draw(truncated_row(s, samp, kw), rng_uniform(seed, st, r))
    c = count(row, plen, ras[0], x) if ras and ras[0] > 0 else 0
    out = dict(x=x, tok=x, redraw=False, margin1=m1, margin2=float("inf"), c=c)
    if ras and ras[0] > 0 and c >= ras[1] and x != eos and not finished and not full:
        out["tok"], out["margin2"] = draw(s, rng_uniform(seed ^ SALT, st, r))
        out["redraw"] = True
    if finished or full:
        out["tok"] = eos
    return out
