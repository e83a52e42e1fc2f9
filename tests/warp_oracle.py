"""Test infrastructure: the typical / epsilon / eta sampling warpers of include/genvc_hip.h (gvc_logits_warpers) restated on the CPU, one
row at a time, and the sampler loop of the fixture cases (tests/golden/logits_warpers.npz) built on them.  Order, as transformers'
_get_logits_processor builds it and the device applies it:
  repetition penalty -> [processors] -> temperature -> top_k -> top_p -> min_p -> typical -> epsilon -> eta -> draw.
Masked ids are -inf; every warper sees the scores the previous one left, probabilities renormalised over the survivors."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import proc_oracle as PO      # noqa: E402

KEYS = ("typical_p", "epsilon_cutoff", "eta_cutoff")
NEG = -float("inf")


def entropy(s):
    """-sum p log p over the finite entries of s [V] (HF: log_softmax + nansum, Categorical(logits).entropy())"""
    logp = torch.log_softmax(s, -1)
    p = torch.exp(logp)
    return -(logp * p).nansum(-1)


def typical_keys(s):
    """(key |-logp - H| per id, p per id) of scores s [V]"""
    logp = torch.log_softmax(s, -1)
    p = torch.exp(logp)
    H = -(logp * p).nansum(-1)
    return torch.abs(-logp - H), p


def typical_threshold(s, mass):
    """T: the smallest key at which the mass of the ids with key <= T reaches `mass` (the largest surviving key if none does)"""
    key, p = typical_keys(s)
    alive = torch.isfinite(s)
    k = key[alive].double().numpy()
    q = p[alive].double().numpy()
    order = np.argsort(k, kind="stable")
    k, q = k[order], q[order]
    cum = np.cumsum(q)
    for i in range(len(k)):
        if i + 1 < len(k) and k[i + 1] == k[i]:
            continue                       # (the mass at or below a key counts its whole tie group)
        if cum[i] >= mass:
            return float(k[i])
    return float(k[-1])


def typical_keep(s, mass):
    """TypicalLogitsWarper(mass): every id with key <= T (ties included)"""
    key, _ = typical_keys(s)
    return torch.isfinite(s) & (key.double() <= typical_threshold(s, mass))


def epsilon_keep(s, eps):
    """EpsilonLogitsWarper(eps): p >= eps, or the score equals the largest"""
    p = torch.softmax(s, -1)
    return torch.isfinite(s) & ~((p < eps) & (s < s.max()))


def eta_keep(s, eps):
    """EtaLogitsWarper(eps): the epsilon rule with min(eps, sqrt(eps) exp(-H))"""
    e = torch.tensor(eps, dtype=torch.float32)
    eta = torch.min(e, torch.sqrt(e) * torch.exp(-entropy(s)))
    p = torch.softmax(s, -1)
    return torch.isfinite(s) & ~((p < eta) & (s < s.max()))


def on_values(kw):
    """the warpers transformers builds for these kwargs with do_sample=True, as (name, value) in order; ValueError where it raises"""
    out = []
    t = kw.get("typical_p")
    if t is not None and float(t) < 1.0:
        if not float(t) > 0.0:
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {t}")
        out.append(("typical_p", float(t)))
    for k in ("epsilon_cutoff", "eta_cutoff"):
        v = kw.get(k)
        if v is not None and 0.0 < float(v) < 1.0:
            out.append((k, float(v)))
    return out


def warp(s, kw):
    """typical -> epsilon -> eta on scores s [V] (after min_p) -> the warped scores (dropped ids -inf)"""
    fns = {"typical_p": typical_keep, "epsilon_cutoff": epsilon_keep, "eta_cutoff": eta_keep}
    for k, v in on_values(kw):
        s = torch.where(fns[k](s, v), s, torch.full_like(s, NEG))
    return s


def margins(s, kw):
    """the screens of a fixture step on scores s [V] (after min_p, before the warpers) -> (ids that survive every warper, typical: how
    far the mass at or below the threshold T -- and below it -- lies from typical_p, typical: key gap between T and its neighbours,
    cutoffs: cutoff - the largest p of the ids other than the top one), each inf when that warper is off.  A single survivor of
    typical alone gives (1, p - typical_p, gap to the next key, inf)."""
    typ = gap = cut = np.inf
    x = s
    for k, v in on_values(kw):
        if k == "typical_p":
            # the threshold's tie group must hold the mass clear of v on both sides, and its key must stand clear of its neighbours
            key, p = typical_keys(x)
            alive = torch.isfinite(x)
            T = typical_threshold(x, v)
            kd, pd = key[alive].double(), p[alive].double()
            below, upto = float(pd[kd < T].sum()), float(pd[kd <= T].sum())
            typ = min(typ, upto - v, v - below)
            lo, hi = kd[kd < T], kd[kd > T]
            if len(lo):
                gap = min(gap, T - float(lo.max()))
            if len(hi):
                gap = min(gap, float(hi.min()) - T)
            x = torch.where(typical_keep(x, v), x, torch.full_like(x, NEG))
        else:
            p = torch.softmax(x, -1)
            thr = v
            if k == "eta_cutoff":
                e = torch.tensor(v, dtype=torch.float32)
                thr = float(torch.min(e, torch.sqrt(e) * torch.exp(-entropy(x))))
            top = int(torch.argmax(x))
            others = torch.cat([p[:top], p[top + 1:]])
            cut = min(cut, thr - float(others.max()))
            x = torch.where(eta_keep(x, v) if k == "eta_cutoff" else epsilon_keep(x, v), x, torch.full_like(x, NEG))
    return int(torch.isfinite(x).sum()), typ, gap, cut


def pre_warp(s, row, rep, temp, top_k, top_p):
    """repetition penalty -> temperature -> top_k -> top_p on the raw logits s [V] of a row (transformers' warper classes for the
    three in the middle) -> the scores the warpers see"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    x = PO.rep_penalty(s.float(), row, rep)[None]
    if temp != 1.0:
        x = TemperatureLogitsWarper(temp)(None, x)
    if top_k:
        x = TopKLogitsWarper(top_k)(None, x)
    if top_p < 1.0:
        x = TopPLogitsWarper(top_p)(None, x)
    return x[0]


@torch.inference_mode()
def single_survivor(ora, cond, codes, kw, samp, max_new):
    """the sampler loop of a fixture case: at every live step exactly one id must survive the warpers, so the draw is that id ->
    (tokens [B, n] int64 padded with eos after a row stops, per-step margins [B, n, 4] (see margins(); inf once the row has stopped),
    argmax [B, n]: the largest pre-warper score's id)"""
    eos = ora.dims["stop_audio_token"]
    fake, logits, cache = ora.prefill(cond, codes)
    B = fake.shape[0]
    rows = [list(map(int, r)) for r in fake]
    fin = [False] * B
    toks, marg, amax = [], [], []
    for t in range(max_new):
        tok, mg, am = [], [], []
        for b in range(B):
            x = pre_warp(logits[b], rows[b], samp["repetition_penalty"], samp["temperature"], samp["top_k"], samp["top_p"])
            n, a, g, c = margins(x, kw)
            y = warp(x, kw)
            pick = int(torch.argmax(y))
            if fin[b]:
                pick, n, a, g, c = eos, 1, np.inf, np.inf, np.inf
            mg.append((n, a, g, c))
            am.append(int(torch.argmax(x)))
            tok.append(pick)
            rows[b].append(pick)
            fin[b] = fin[b] or pick == eos
        toks.append(tok)
        marg.append(mg)
        amax.append(am)
        if all(fin):
            break
        logits, cache = ora.step(cache, torch.tensor(tok), t + 1)
    return np.array(toks, dtype=np.int64).T, np.array(marg, dtype=np.float64).transpose(1, 0, 2), np.array(amax, dtype=np.int64).T
