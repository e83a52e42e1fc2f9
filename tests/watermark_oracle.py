"""Test infrastructure: the green-list watermark of include/genvc_hip.h (gvc_logits_watermark, gvc_wm_score) restated on
the CPU, on top of tests/penalty_oracle.py and tests/ras_oracle.py: the table builder, the processor step on one scores row in fp32, the
sampler step with the mark at its place in the chain, and the detector's counts and statistics.

The table: transformers' recipe with a CPU torch.Generator, restated here independently of genvc_amd.engine.watermark_table (sets of
ids, no bit packing); tests/test_watermark_host.py pins both to the installed WatermarkLogitsProcessor(vocab, "cpu", ...).
The step: the row as the chain leaves it behind the last warper (dropped ids -inf); every finite id that is green gains the bias, one
fp32 add; selfhash: only the green ids among the 40 highest scores of the row (transformers' order: a descending sort; ties at rank 40
are the caller's to screen out).  The draw then takes its weights from the biased row relative to its maximum (RO.draw).
Greedy search: argmax of the processed row (no Temperature) with the bias on the green ids."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import penalty_oracle as PN   # noqa: E402
import ras_oracle as RO       # noqa: E402

MARGIN = RO.MARGIN
NEG = -float("inf")
DEFAULT_KEY = 15485863
FIXED_TABLE = 1_000_003
TOP = 40
MOD = 2 ** 64 - 1
_cache = {}


def green_ids(V, key, ratio, prev):
    """lefthash: the green ids after `prev` as a sorted list"""
    g = torch.Generator(device="cpu")
    g.manual_seed((key * prev) % MOD)
    return sorted(torch.randperm(V, generator=g)[:int(V * ratio)].tolist())


def lefthash_lists(V, key, ratio):
    """[V] sets: the green ids after every prev"""
    ck = ("left", V, key, ratio)
    if ck not in _cache:
        _cache[ck] = [set(green_ids(V, key, ratio, p)) for p in range(V)]
    return _cache[ck]


def selfhash_set(V, key, ratio):
    """the ids that are green after themselves (context_width 1: the seed comes from the candidate alone).  The products are int64
    tensor arithmetic and wrap, as transformers' do"""
    ck = ("self", V, key, ratio)
    if ck not in _cache:
        g = torch.Generator(device="cpu")
        g.manual_seed(key)
        fixed = torch.randperm(FIXED_TABLE, generator=g)
        out = set()
        for c in range(V):
            a = fixed[torch.tensor([c]) % FIXED_TABLE] + 1
            seed = (key * a * a).min().item()
            g.manual_seed(seed % MOD)
            if c in torch.randperm(V, generator=g)[:int(V * ratio)].tolist():
                out.add(c)
        _cache[ck] = out
    return _cache[ck]


def green_mask(V, wm, prev):
    """wm = dict(key, ratio, scheme, bias) -> bool [V]: the green list of a step whose previous id is prev; None when the step carries
    no mark (lefthash with prev outside [0, V))"""
    if wm["scheme"] == "selfhash":
        ids = selfhash_set(V, wm["key"], wm["ratio"])
    elif 0 <= prev < V:
        ids = lefthash_lists(V, wm["key"], wm["ratio"])[prev]
    else:
        return None
    m = torch.zeros(V, dtype=torch.bool)
    m[torch.tensor(sorted(ids), dtype=torch.long)] = True
    return m


def rank_tie(s, top=TOP):
    """the row has a tie across rank `top` of its descending order (finite scores only): transformers then picks by sort order, the
    device keeps every tied id -- such rows are screened out of selfhash comparisons"""
    v = torch.sort(s, descending=True)[0]
    return s.numel() > top and bool(torch.isfinite(v[top - 1])) and bool(v[top - 1] == v[top])


def mark_row(s, wm, prev):
    """the processor step on one scores row s [V] fp32 (dropped ids -inf) -> the biased row"""
    V = s.numel()
    g = green_mask(V, wm, prev) if wm is not None else None
    if g is None:
        return s.clone()
    if wm["scheme"] == "selfhash":
        v = torch.sort(s, descending=True)[0]
        g = g & (s >= v[min(TOP, V) - 1])
    g = g & torch.isfinite(s)
    return torch.where(g, s + torch.tensor(wm["bias"], dtype=torch.float32), s)          # fl(score + bias)


def step(logits, row, plen, samp, kw, wm, key, eos, pen=None, finished=False, full=False, greedy_search=False):
    """one sampler step of one row with the mark behind the last warper.  greedy_search: do_sample=False -- the argmax of the processed
    row (divided by the call's temperature, which a greedy search with the mark sets to 1) with the bias.
    -> dict(tok, margin1, scores: the row the token is taken from)"""
    prev = row[-1] if row else -1
    seed, st, r = key
    if samp["top_k"] == 1 or greedy_search:
        s = PN.full_row(logits, row, plen, samp, kw, eos, pen)
        if wm is not None:
            s = _self_all(s, wm) if wm["scheme"] == "selfhash" else mark_row(s, wm, prev)
        tok, m1 = int(torch.argmax(s)), float("inf")
    else:
        s = PN.full_row(logits, row, plen, samp, kw, eos, pen)
        s = mark_row(RO.truncated_row(s, samp, kw), wm, prev)
        tok, m1 = RO.draw(s, RO.rng_uniform(seed, st, r))
    if finished or full:
        tok = eos
    return dict(tok=tok, margin1=m1, scores=s)


def _self_all(s, wm):
    """the device's top_k == 1 rule under selfhash (documented as not transformers' and refused by the Python layer): every self-green
    id gains the bias"""
    g = green_mask(s.numel(), wm, 0) & torch.isfinite(s)
    return torch.where(g, s + torch.tensor(wm["bias"], dtype=torch.float32), s)


def detector_flags(codes, length, V, wm, ignore_repeated=False):
    """codes: a list of ids, `length` of them valid -> (scored, green, flags list over all of codes: 1 green, 0 scored and not green,
    2 unscored)"""
    selfhash = wm["scheme"] == "selfhash"
    flags, seen = [], set()
    for t, cur in enumerate(codes):
        f = 2
        if t < length and (selfhash or t >= 1):
            prev = 0 if selfhash else codes[t - 1]
            ok = 0 <= cur < V and (selfhash or 0 <= prev < V)
            gram = (cur,) if selfhash else (prev, cur)
            if ok and not (ignore_repeated and gram in seen):
                seen.add(gram)
                g = selfhash_set(V, wm["key"], wm["ratio"]) if selfhash else lefthash_lists(V, wm["key"], wm["ratio"])[prev]
                f = int(cur in g)
        flags.append(f)
    return sum(f != 2 for f in flags), sum(f == 1 for f in flags), flags


def statistics(scored, green, ratio):
    """transformers' z and p in float64 (numpy scalars, HF's operation order)"""
    scored, green = np.float64(scored), np.float64(green)
    with np.errstate(divide="ignore", invalid="ignore"):          # (nothing scored: z is nan, as the division says)
        z = (green - ratio * scored) / np.sqrt(scored * ratio * (1 - ratio))
        p = 1 - (0.5 * (1 + np.sign(z) * (1 - np.exp(-2 * z ** 2 / np.pi))))
    return float(z), float(p)
