"""Test infrastructure: speculative sampling (include/genvc_hip.h: gvc_spec_accept_sample, gvc_gpt_generate_assisted_sample) restated
on the CPU in float64.

`warp` is the row a sampler step draws from: oracle.process_logits for the repetition penalty, tests/proc_oracle.py's processors at
the row's length, oracle.process_logits again for Temperature / TopK / TopP, then MinP.  `draw` is oracle.sample_from_scores' rule on
explicit weights.  `accept` restates the accept step of one round on numpy state (the fields of tests/assist_oracle.py: accept) and
returns the margin of every decision it took: the relative CDF distance of a draw (as _draw of tests/test_gpu_row_sampling.py), and
|r q - p| / max(r q, p) of an accept test.  `generate` chains rounds of a draft and a target oracle model into a whole generation.
Uniforms: u_draft(t) = rng_uniform(seed, t, 3b), u_acc(t) = rng_uniform(seed, t, 3b + 1), u_res(t) = rng_uniform(seed, t, 3b + 2), t the
0-based index of the token being decided."""
import os
import sys

import math

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import proc_oracle as PO                          # noqa: E402
from oracle import genvc_oracle as O              # noqa: E402

INF = float("inf")


def u_draft(seed, t, b):
    return O.rng_uniform(seed, t, 3 * b)


def u_acc(seed, t, b):
    return O.rng_uniform(seed, t, 3 * b + 1)


def u_res(seed, t, b):
    return O.rng_uniform(seed, t, 3 * b + 2)


def warp(logits_row, row, plen, kw, samp, eos, sets=None, a=0.0):
    """fp32 logits [V] and the input_ids row (list) -> the warped scores [V] fp32, dropped entries -inf.  sets: a list that receives the
    margins of the kept set's own decisions against warped scores that move by up to `a` (see generate): the gap between the last id
    TopK keeps and the first it drops, less 2 a, and the distance of every cumulative mass from TopP's cut 1 - top_p, less the most that
    mass can move"""
    ids = torch.tensor([row], dtype=torch.long)
    s = O.process_logits(torch.as_tensor(logits_row).float()[None], ids, samp["repetition_penalty"], 1.0, 0, 1.0)[0]
    s = PO.process(s, row, plen, kw, eos)
    if sets is not None:
        t = s / samp["temperature"]
        k = samp["top_k"]
        if k and 0 < k < t.numel():
            top = torch.topk(t, k + 1)[0]
            sets.append(float(top[k - 1] - top[k]) - 2.0 * a)
            t = t.masked_fill(t < top[k - 1], -INF)
        if samp["top_p"] < 1.0:
            cp = torch.sort(t)[0].double().softmax(-1).cumsum(-1)[:-1]
            cp = cp[cp > 0]
            sets.append(float(((cp - (1.0 - samp["top_p"])).abs() - math.expm1(2.0 * a) * cp * (1.0 - cp)).min()))
    s = O.process_logits(s[None], ids, 1.0, samp["temperature"], samp["top_k"], samp["top_p"])[0]
    if kw.get("min_p"):
        s = s.masked_fill(~PO.min_p_keep(s, float(kw["min_p"])), -INF)
    return s


def weights(s):
    """warped scores -> (float64 weights expf(s - max) of the kept entries, computed in fp32 as the sampler does; kept mask)"""
    kept = torch.isfinite(s)
    e = torch.where(kept, torch.exp(s - s[kept].max()), torch.zeros_like(s))
    return e.double().numpy(), kept.numpy()


def draw(w, kept, u, a=0.0, slack=None):
    """the first kept index whose running mass (float64, vocabulary order) reaches u * total, else the last kept index; and the
    draw's relative distance to the nearest CDF boundary.  a: the warped scores may move by up to a, a weight then by a factor in
    [e^-a, e^a] and a CDF value F = C / (C + R) by at most (e^2a - 1) F (1 - F), which comes off the distance.  slack: per-boundary
    allowances instead (the residual)"""
    cdf = np.cumsum(w)
    total = float(cdf[-1])
    target = float(np.float32(u)) * total
    hit = np.nonzero((cdf >= target) & kept)[0]
    tok = int(hit[0]) if len(hit) else int(np.nonzero(kept)[0][-1])
    F = cdf[kept] / total
    move = math.expm1(2.0 * a) * F * (1.0 - F) if slack is None else slack[kept]
    return tok, float((np.abs(F - target / total) - move).min())


def decide(p_scores, q_scores, x, r, u, a=0.0, a_res=0.0):
    """one position of the rule.  q_scores None: draw from p with u.  -> (token, accepted, margins).  a: as in draw; a probability then
    moves by a factor within e^+-2a, both sides of the accept test together by e^+-4a.  a_res: the same for the residual, where a CDF
    value C / R moves by what |delta (p_j - q_j)| <= (e^2a - 1) (p_j + q_j) sums to in C and in R"""
    wp, kp = weights(p_scores)
    if q_scores is None:
        tok, mg = draw(wp, kp, u, a)
        return tok, False, [mg]
    wq, _ = weights(q_scores)
    p, q = wp / wp.sum(), wq / wq.sum()          # (np.sum pairs terms; the totals differ from a running sum far below the margins)
    lhs, rhs = float(np.float32(r)) * q[x], p[x]
    mg = abs(lhs - rhs) / max(lhs, rhs) - (-math.expm1(-4.0 * a)) if max(lhs, rhs) > 0 else INF
    if lhs <= rhs:
        return int(x), True, [mg]
    res = np.maximum(p - q, 0.0)
    if res.sum() > 0:
        slack = None
        if a_res > 0.0:
            e = math.expm1(2.0 * a_res) * (p + q)
            C, E, R, EV = np.cumsum(res), np.cumsum(e), res.sum(), e.sum()
            hi, lo = (C + E) / max(R - EV, 1e-300), (C - E) / (R + EV)
            slack = np.maximum(hi - C / R, C / R - lo)
        tok, m2 = draw(res, res > 0, u, slack=slack)
    else:
        tok, m2 = draw(wp, kp, u, a)
    return tok, False, [mg, m2]


def draft(logits, ids, ids_len, emitted, finished, k, samp, seed, eos, kw=None, plen=0, max_new=None):
    """the draft side of one round on given draft logits [B, k, V] (row j: the draft model's output behind [.., d_1..d_j]): ->
    (drafts int32 [B, k], q_scores fp32 [B, k + 1, V] with row j + 1 the row d_{j+1} was drawn from, margins)"""
    kw = kw or {}
    B, _, V = logits.shape
    drafts = np.full((B, k), eos, dtype=np.int32)
    q = np.full((B, k + 1, V), -INF, dtype=np.float32)
    margins = []
    for b in range(B):
        if finished[b]:
            continue
        row = [int(x) for x in ids[b, :ids_len[b]]]
        for j in range(k):
            s = warp(logits[b, j], row, plen, kw, samp, eos)
            q[b, j + 1] = s.numpy()
            w, kept = weights(s)
            tok, mg = draw(w, kept, u_draft(seed, int(emitted[b]) + j, b))
            if max_new is None or j < max_new - int(emitted[b]) - 1:
                margins.append(mg)
            drafts[b, j] = tok
            row.append(tok)
            if tok == eos:
                break          # (the sampler pads a finished row with the stop token; nothing behind it is read)
    return drafts, q, margins


def accept(st, k, appended, logits, latents, drafts, q_scores, samp, seed, eos, kw=None, plen=0):
    """One accept step of speculative sampling on numpy state, in place (st as tests/assist_oracle.py: accept).  logits [B, k + 1, V],
    latents [B, k + 1, d], drafts [B, >= k] (None for k = 0), q_scores [B, k + 1, V] (None for k = 0).  -> dict(margins, accepts,
    rejects, p: the warped target rows [B, k + 1, V], nan where the step did not warp)"""
    kw = kw or {}
    B, _, V = logits.shape
    out = dict(margins=[], accepts=0, rejects=0, p=np.full((B, k + 1, V), np.nan, dtype=np.float32))
    for b in range(B):
        len0, em0 = int(st["ids_len"][b]), int(st["emitted"][b])
        if st["finished"][b] or em0 >= st["max_new"]:
            st["finished"][b] = 1
            st["drop_target"][b] = st["drop_assistant"][b] = appended
            continue
        kk = min(k, st["max_new"] - em0 - 1) if drafts is not None else 0
        for j in range(kk):
            st["ids"][b, len0 + j] = drafts[b, j]
        m = acc = 0
        fin = False
        for i in range(kk + 1):
            row = [int(x) for x in st["ids"][b, :len0 + i]]
            p = warp(logits[b, i], row, plen, kw, samp, eos)
            out["p"][b, i] = p.numpy()
            if i < kk:
                tok, ok, mg = decide(p, torch.from_numpy(q_scores[b, i + 1]), int(drafts[b, i]), u_acc(seed, em0 + i, b),
                                     u_res(seed, em0 + i, b))
                out["accepts" if ok else "rejects"] += 1
            else:
                tok, ok, mg = decide(p, None, None, None, u_res(seed, em0 + i, b))
            out["margins"] += mg
            st["toks"][b, em0 + m] = tok
            st["ids"][b, len0 + i] = tok
            st["lats"][b, em0 + m] = latents[b, i]
            m += 1
            last = tok
            if tok == eos:
                fin = True
                break
            if ok:
                acc += 1
            else:
                break
        st["ids_len"][b] = len0 + m
        st["emitted"][b] = em0 + m
        st["pending"][b] = last
        st["finished"][b] = 1 if fin or em0 + m >= st["max_new"] else 0
        st["drop_target"][b] = st["drop_assistant"][b] = appended - m if appended > 0 else 0
        if appended > 0:
            st["rounds"][b] += 1
            st["drafted"][b] += kk
            st["accepted"][b] += acc
    return out


class _Model:
    """one oracle GPT decoding ONE stream, with every cache it has produced kept: position n is re-entered after a rollback by
    feeding token n on the cache of the n tokens before it"""

    def __init__(self, w, dims, cond, codes):
        self.w = {k: (v if torch.is_tensor(v) else torch.as_tensor(v)).float() for k, v in w.items()}
        self.dims = dims
        prefix, fake = O.compute_embeddings(self.w, dims, cond.float(), codes.long())
        z, logits, cache = O.gpt_prefill(self.w, dims, prefix)
        self.fake = [int(x) for x in fake[0]]
        self.out = {(): (z[0], logits[0], cache)}

    def after(self, toks):
        """(latent, logits) behind the generated tokens `toks` (a tuple)"""
        toks = tuple(int(t) for t in toks)
        if toks not in self.out:
            self.after(toks[:-1])
            cache = self.out[toks[:-1]][2]
            z, logits, cache = O.gpt_decode_step(self.w, self.dims, cache, torch.tensor([toks[-1]]), len(toks))
            self.out[toks] = (z[0], logits[0], cache)
        return self.out[toks][:2]


@torch.inference_mode()
def generate(tw, tdims, dw, ddims, cond, codes, k, samp, seed, max_new, kw=None, logit_screen=0.0, logit_tol=0.0, need=None):
    """speculative sampling of B streams on the CPU: target weights tw, draft weights dw, both with the call's settings.  ->
    dict(ids [B, n] int64 padded with the stop token, latents [B, n, d], margins: every decision's, floor: the smallest, rounds /
    drafted / accepted [B]).
    The margins are what is left of them when the logits of both models move by up to delta, i.e. a warped score by up to a =
    repetition_penalty * delta / temperature, worked out per decision (no first-order shortcuts: `draw`, `decide`, `warp`).  delta =
    logit_screen for the draws from a warped row and the accept tests; delta = logit_tol for the residual draws and for the kept sets'
    own decisions (TopK's last gap, TopP's cut), whose margins join the list when logit_tol > 0.  need: give up (return None) at
    the first round that leaves a margin at or below it -- a seed search spends little on the seeds it drops"""
    kw = kw or {}
    a = samp["repetition_penalty"] * logit_screen / samp["temperature"]
    at = samp["repetition_penalty"] * logit_tol / samp["temperature"]
    eos = tdims["stop_audio_token"]
    B = cond.shape[0]
    rows_t, lat_rows, margins = [], [], []
    sets = margins if logit_tol > 0.0 else None
    stats = np.zeros((3, B), dtype=np.int64)
    for b in range(B):
        T, D = _Model(tw, tdims, cond[b:b + 1], codes[b:b + 1]), _Model(dw, ddims, cond[b:b + 1], codes[b:b + 1])
        n0 = len(T.fake)
        z, lg = T.after(())
        tok, _, mg = decide(warp(lg, T.fake, n0, kw, samp, eos, sets, at), None, None, None, u_res(seed, 0, b), a, at)
        margins += mg
        toks, lats = [tok], [z]
        while toks[-1] != eos and len(toks) < max_new:
            e = len(toks)
            kk = min(k, max_new - e - 1)
            drafts, qs = [], []
            for j in range(kk):
                if drafts and drafts[-1] == eos:
                    drafts.append(eos)
                    qs.append(None)
                    continue
                _, lg = D.after(toks + drafts)
                q = warp(lg, D.fake + toks + drafts, n0, kw, samp, eos, sets, at)
                w, kept = weights(q)
                d, mg = draw(w, kept, u_draft(seed, e + j, b), a)
                margins.append(mg)
                drafts.append(d)
                qs.append(q)
            stats[0, b] += 1
            stats[1, b] += kk
            have = list(toks)          # (the accepted drafts join toks as the loop goes)
            for i in range(kk + 1):
                z, lg = T.after(have + drafts[:i])
                p = warp(lg, T.fake + have + drafts[:i], n0, kw, samp, eos, sets, at)
                if i < kk:
                    tok, ok, mg = decide(p, qs[i], drafts[i], u_acc(seed, e + i, b), u_res(seed, e + i, b), a, at)
                else:
                    tok, ok, mg = decide(p, None, None, None, u_res(seed, e + i, b), a, at)
                margins += mg
                toks.append(tok)
                lats.append(z)
                if tok == eos or not ok:
                    break
                stats[2, b] += 1
            if need is not None and min(margins) <= need:
                return None
        rows_t.append(toks)
        lat_rows.append(torch.stack(lats))
    n = max(len(r) for r in rows_t)
    ids = np.full((B, n), eos, dtype=np.int64)
    lat = torch.zeros(B, n, lat_rows[0].shape[-1])
    for b, r in enumerate(rows_t):
        ids[b, :len(r)] = r
        lat[b, :len(r)] = lat_rows[b]
    if need is not None and min(margins) <= need:
        return None
    return dict(ids=ids, latents=lat, margins=margins, floor=min(margins), rounds=stats[0], drafted=stats[1], accepted=stats[2])


# ---- the distribution case: 64 seeds x 64 identical rows, V = 32, no truncation, one round with one draft at position 1 ------------------
DIST_V, DIST_EOS, DIST_B, DIST_SEEDS, DIST_N0 = 32, 31, 64, tuple(range(1000, 1064)), 4
DIST_SAMP = dict(repetition_penalty=1.0, temperature=1.0, top_k=0, top_p=1.0)


def chi2_bound(dof):
    """the chi-square 0.999 quantile by Wilson-Hilferty"""
    return dof * (1.0 - 2.0 / (9.0 * dof) + 3.0902 * (2.0 / (9.0 * dof)) ** 0.5) ** 3


def dist_case(disjoint=False):
    """-> dict(logits fp32 [2, V]: the target's rows 0 and 1 of every stream, draft_logits fp32 [V], samp).  disjoint: top_k = 15 and a
    draft whose 15 best ids are the target's 15 worst"""
    from genvc_amd import synth
    t = synth.uniform(71, "spec_dist_target", (2, DIST_V), 1.5 / 3 ** 0.5).float()          # (scale is a deviation: amplitude +-1.5)
    if disjoint:
        return dict(logits=t, draft_logits=-t[0], samp=dict(DIST_SAMP, top_k=15))
    return dict(logits=t, draft_logits=t[0] + synth.uniform(72, "spec_dist_draft", (DIST_V,), 1.0 / 3 ** 0.5).float(), samp=DIST_SAMP)


def dist_round(case, seed):
    """one call of the distribution case on the CPU: -> (drafts int32 [B, 1], q_scores fp32 [B, 2, V], first tokens [B], the smallest
    margin of each row's decisions [B], accepted flags [B], p_0 as probabilities float64 [V])"""
    row = [1] * DIST_N0 + [0]          # the prompt and the opening token: every row has emitted one token
    samp = case["samp"]
    q0 = warp(case["draft_logits"], row, DIST_N0, {}, samp, DIST_EOS)
    p0 = warp(case["logits"][0], row, DIST_N0, {}, samp, DIST_EOS)
    wq, kq = weights(q0)
    wp, _ = weights(p0)
    drafts = np.zeros((DIST_B, 1), dtype=np.int32)
    q = np.full((DIST_B, 2, DIST_V), -INF, dtype=np.float32)
    q[:, 1] = q0.numpy()
    toks, floor, acc = np.zeros(DIST_B, dtype=np.int64), np.zeros(DIST_B), np.zeros(DIST_B, dtype=bool)
    for b in range(DIST_B):
        drafts[b, 0], _ = draw(wq, kq, u_draft(seed, 1, b))
        toks[b], acc[b], mg = decide(p0, q0, int(drafts[b, 0]), u_acc(seed, 1, b), u_res(seed, 1, b))
        floor[b] = min(mg)
    return drafts, q, toks, floor, acc, wp / wp.sum()


def chi2(tokens, p):
    """Pearson's statistic of a token histogram against probabilities p over the ids with p > 0 -> (chi2, dof, smallest expected count,
    tokens outside the support)"""
    n = len(tokens)
    cnt = np.bincount(np.asarray(tokens), minlength=len(p)).astype(np.float64)
    on = p > 0
    exp = n * p[on]
    return float(((cnt[on] - exp) ** 2 / exp).sum()), int(on.sum()) - 1, float(exp.min()), int(cnt[~on].sum())
