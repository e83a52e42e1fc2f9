"""Test infrastructure: prompt-lookup assisted decoding (GPT.generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=N);
include/genvc_hip.h: gvc_spec_lookup, gvc_spec_accept_len, gvc_spec_accept_sample_len, gvc_gpt_generate_lookup) restated on the CPU.

`lookup` is the rule on one history (a list of generated codes, the last one the pending token); `lookup_rows` applies it to the state
arrays the kernel reads and returns what the kernel writes.  `accept_len` / `accept_sample_len` restate the accept steps with a draft
count per row; their only arithmetic is tests/assist_oracle.py: chain_token and tests/spec_sample_oracle.py: warp / decide.
`generate` chains rounds on one oracle model into a whole generation, greedy or sampled; the sampled chain feeds decide() explicit
one-hot rows (`onehot`), and `decide_onehot` is the same rule in closed form: accept x iff u_acc <= p(x), else draw from p without x."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import assist_oracle as AO                    # noqa: E402
import spec_sample_oracle as SO               # noqa: E402

INF = float("inf")


def lookup(h, k, N):
    """h: the generated codes of one row.  For n = min(N, len - 1) down to 1: the lowest i with h[i:i + n] == h[len - n:] and
    i + n < len; the first n with a hit wins.  -> the drafts h[i + n : i + n + k] (up to the end of h; [] without a hit)"""
    h = [int(x) for x in h]
    L = len(h)
    for n in range(min(N, L - 1), 0, -1):
        suf = h[L - n:]
        for i in range(L - n):
            if h[i:i + n] == suf:
                return h[i + n:min(i + n + k, L)]
    return []


def onehot(tok, V):
    """the one-hot row of a draft as the accept step reads it: warped scores, 0 at the token and -inf elsewhere"""
    q = np.full(V, -INF, dtype=np.float32)
    if 0 <= tok < V:
        q[tok] = 0.0
    return q


def lookup_rows(ids, ids_len, finished, pending, k, N, start, vocab=None):
    """the kernel's outputs for state arrays: -> (v_toks int32 [B, k + 1], draft_len int32 [B], q fp32 [B, k + 1, vocab] or None; row 0
    of q and the rows of finished streams are nan: the kernel leaves them alone)"""
    B = len(ids_len)
    v = np.zeros((B, k + 1), dtype=np.int32)
    dl = np.zeros(B, dtype=np.int32)
    q = None if vocab is None else np.full((B, k + 1, vocab), np.nan, dtype=np.float32)
    for b in range(B):
        v[b, :] = pending[b]
        if finished[b]:
            continue
        d = lookup(ids[b, start:ids_len[b]], k, N)
        dl[b] = len(d)
        v[b, 1:1 + len(d)] = d
        if q is not None:
            for j in range(1, k + 1):
                q[b, j] = onehot(int(v[b, j]), vocab)
    return v, dl, q


def _clamp(k, st, em0, drafts, draft_len, b):
    if drafts is None:
        return 0
    kk = min(k, st["max_new"] - em0 - 1)
    return kk if draft_len is None else min(kk, max(int(draft_len[b]), 0))


def accept_len(st, k, appended, logits, latents, drafts, draft_len, rep, eos, kw=None, plen=0):
    """tests/assist_oracle.py: accept with k' = min(k, max_new - emitted - 1, draft_len[b]); draft_len None: that function's k'"""
    kw = kw or {}
    for b in range(logits.shape[0]):
        len0, em0 = int(st["ids_len"][b]), int(st["emitted"][b])
        if st["finished"][b] or em0 >= st["max_new"]:
            st["finished"][b] = 1
            st["drop_target"][b] = st["drop_assistant"][b] = appended
            continue
        kk = _clamp(k, st, em0, drafts, draft_len, b)
        m = acc = 0
        fin = False
        for i in range(kk + 1):
            if i > 0:
                st["ids"][b, len0 + i - 1] = drafts[b, i - 1]
            row = [int(x) for x in st["ids"][b, :len0 + i]]
            tok, _ = AO.chain_token(logits[b, i], row, plen, kw, rep, eos)
            st["toks"][b, em0 + m] = tok
            st["ids"][b, len0 + i] = tok
            st["lats"][b, em0 + m] = latents[b, i]
            m += 1
            last = tok
            if tok == eos:
                fin = True
                break
            if i < kk and tok == int(drafts[b, i]):
                acc += 1
            else:
                break
        _book(st, b, len0, em0, m, last, fin, appended, kk, acc)
    return st


def _book(st, b, len0, em0, m, last, fin, appended, kk, acc):
    st["ids_len"][b] = len0 + m
    st["emitted"][b] = em0 + m
    st["pending"][b] = last
    st["finished"][b] = 1 if fin or em0 + m >= st["max_new"] else 0
    st["drop_target"][b] = st["drop_assistant"][b] = appended - m if appended > 0 else 0
    if appended > 0:
        st["rounds"][b] += 1
        st["drafted"][b] += kk
        st["accepted"][b] += acc


def accept_sample_len(st, k, appended, logits, latents, drafts, draft_len, q_scores, samp, seed, eos, kw=None, plen=0):
    """tests/spec_sample_oracle.py: accept with k' clamped by draft_len[b] as well (None: that function's k').  -> dict(margins, accepts,
    rejects, p)"""
    kw = kw or {}
    B, _, V = logits.shape
    out = dict(margins=[], accepts=0, rejects=0, p=np.full((B, k + 1, V), np.nan, dtype=np.float32))
    for b in range(B):
        len0, em0 = int(st["ids_len"][b]), int(st["emitted"][b])
        if st["finished"][b] or em0 >= st["max_new"]:
            st["finished"][b] = 1
            st["drop_target"][b] = st["drop_assistant"][b] = appended
            continue
        kk = _clamp(k, st, em0, drafts, draft_len, b)
        for j in range(kk):
            st["ids"][b, len0 + j] = drafts[b, j]
        m = acc = 0
        fin = False
        for i in range(kk + 1):
            row = [int(x) for x in st["ids"][b, :len0 + i]]
            p = SO.warp(logits[b, i], row, plen, kw, samp, eos)
            out["p"][b, i] = p.numpy()
            if i < kk:
                tok, ok, mg = SO.decide(p, torch.from_numpy(q_scores[b, i + 1]), int(drafts[b, i]), SO.u_acc(seed, em0 + i, b),
                                        SO.u_res(seed, em0 + i, b))
                out["accepts" if ok else "rejects"] += 1
            else:
                tok, ok, mg = SO.decide(p, None, None, None, SO.u_res(seed, em0 + i, b))
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
        _book(st, b, len0, em0, m, last, fin, appended, kk, acc)
    return out


def decide_onehot(p_scores, x, r, u):
    """speculative sampling with q = one-hot at x, in closed form: accept x iff float32(r) <= p(x); else one token from p with x
    removed (from p itself when that is empty) by the sampler's inverse-CDF rule with u.  -> (token, accepted)"""
    wp, kp = SO.weights(p_scores)
    p = wp / wp.sum()
    if float(np.float32(r)) <= p[x]:
        return int(x), True
    res = p.copy()
    res[x] = 0.0
    if res.sum() > 0:
        return SO.draw(res, res > 0, u)[0], False
    return SO.draw(wp, kp, u)[0], False


@torch.inference_mode()
def generate(tw, tdims, cond, codes, k, N, max_new, samp=None, seed=0, kw=None, rep=1.0, logit_screen=0.0, logit_tol=0.0, need=None):
    """prompt-lookup assisted decoding of B streams on the CPU, one oracle model.  samp None: greedy (the chain of
    tests/assist_oracle.py at repetition penalty `rep`); samp: speculative sampling with one-hot draft rows on the uniforms of
    tests/spec_sample_oracle.py (u_draft unused), margins as in its generate (logit_screen / logit_tol / need).
    -> dict(ids [B, n] int64 padded with the stop token, latents [B, n, d], rounds / drafted / accepted int64 [B], hits: rounds of
    each row with at least one draft; sampled also margins, floor)"""
    kw = kw or {}
    eos = tdims["stop_audio_token"]
    V = tdims["num_audio_tokens"]
    B = cond.shape[0]
    a = at = 0.0
    margins = []
    if samp is not None:
        a = samp["repetition_penalty"] * logit_screen / samp["temperature"]
        at = samp["repetition_penalty"] * logit_tol / samp["temperature"]
    sets = margins if samp is not None and logit_tol > 0.0 else None
    rows_t, lat_rows = [], []
    stats = np.zeros((4, B), dtype=np.int64)

    def token(T, n0, gen, t, b, q, x):
        """decide token t of row b behind the generated ids `gen`: -> (token, accepted, latent)"""
        z, lg = T.after(gen)
        if samp is None:
            tok, _ = AO.chain_token(lg, T.fake + gen, n0, kw, rep, eos)
            return tok, x is not None and tok == x, z
        p = SO.warp(lg, T.fake + gen, n0, kw, samp, eos, sets, at)
        if x is None:
            tok, ok, mg = SO.decide(p, None, None, None, SO.u_res(seed, t, b), a, at)
        else:
            tok, ok, mg = SO.decide(p, torch.from_numpy(q), x, SO.u_acc(seed, t, b), SO.u_res(seed, t, b), a, at)
        margins.extend(mg)
        return tok, ok, z

    for b in range(B):
        T = SO._Model(tw, tdims, cond[b:b + 1], codes[b:b + 1])
        n0 = len(T.fake)
        tok, _, z = token(T, n0, [], 0, b, None, None)
        toks, lats = [tok], [z]
        while toks[-1] != eos and len(toks) < max_new:
            e = len(toks)
            drafts = lookup(toks, k, N)
            kk = min(k, max_new - e - 1, len(drafts))
            stats[0, b] += 1
            stats[1, b] += kk
            stats[3, b] += len(drafts) > 0
            have = list(toks)
            for i in range(kk + 1):
                x = drafts[i] if i < kk else None
                tok, ok, z = token(T, n0, have + drafts[:i], e + i, b, None if x is None else onehot(x, V), x)
                toks.append(tok)
                lats.append(z)
                if tok == eos or not ok:
                    break
                stats[2, b] += 1
            if need is not None and margins and min(margins) <= need:
                return None
        rows_t.append(toks)
        lat_rows.append(torch.stack(lats))
    n = max(len(r) for r in rows_t)
    ids = np.full((B, n), eos, dtype=np.int64)
    lat = torch.zeros(B, n, lat_rows[0].shape[-1])
    for b, r in enumerate(rows_t):
        ids[b, :len(r)] = r
        lat[b, :len(r)] = lat_rows[b]
    out = dict(ids=ids, latents=lat, rounds=stats[0], drafted=stats[1], accepted=stats[2], hits=stats[3])
    if samp is not None:
        out.update(margins=margins, floor=min(margins))
    return out
