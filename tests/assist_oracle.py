"""Test infrastructure: assisted (speculative) greedy decoding restated on the CPU.

`greedy` is the plain greedy loop of tests/proc_oracle.py on the oracle's GPT forward (tests/beam_oracle.py: OracleGpt) that also keeps
the latent every token was chosen from: assisted greedy decoding must return exactly its tokens, whatever the assistant drafts.
`chain_token` is one position of that loop (repetition penalty, processors, argmax), and `accept` restates the accept step of a round
(include/genvc_hip.h: gvc_spec_accept) on numpy arrays, position by position, with `chain_token` as its only arithmetic."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import beam_oracle as BO      # noqa: E402
import proc_oracle as PO      # noqa: E402

O = BO.O


def chain_token(logits_row, row, plen, kw, rep, eos):
    """the greedy chain on one fp32 logits row [V] against the input_ids row (list): -> (token, top-1 / top-2 margin)"""
    s = PO.process(PO.rep_penalty(torch.as_tensor(logits_row).float(), row, rep), row, plen, kw, eos)
    t2 = torch.topk(s, 2)[0]
    return int(torch.argmax(s)), float(t2[0] - t2[1])


@torch.inference_mode()
def greedy(ora, cond, codes, kw=None, rep=1.0, max_new=12):
    """-> dict(ids [B, n] int64 padded with eos once a row has stopped (n: up to the step where the last row stops), latents [B, n, d],
    margins [B, n], inf once a row has stopped)"""
    kw = kw or {}
    w, dims = ora.w, ora.dims
    eos = dims["stop_audio_token"]
    prefix, fake = O.compute_embeddings(w, dims, cond.float(), codes.long())
    z, logits, cache = O.gpt_prefill(w, dims, prefix)
    B, n0 = fake.shape
    rows = [list(map(int, r)) for r in fake]
    fin = [False] * B
    toks, gaps, lats = [], [], []
    for t in range(max_new):
        tok, gap = [], []
        for b in range(B):
            x, g = chain_token(logits[b], rows[b], n0, kw, rep, eos)
            gap.append(g if not fin[b] else np.inf)
            if fin[b]:
                x = eos
            tok.append(x)
            rows[b].append(x)
            fin[b] = fin[b] or x == eos
        toks.append(tok)
        gaps.append(gap)
        lats.append(z)
        if all(fin) or t == max_new - 1:
            break
        z, logits, cache = O.gpt_decode_step(w, dims, cache, torch.tensor(tok), t + 1)
    return dict(ids=np.array(toks, dtype=np.int64).T, margins=np.array(gaps).T, latents=torch.stack(lats, 1))


def accept(st, k, appended, logits, latents, drafts, rep, eos, kw=None, plen=0):
    """One accept step on numpy state, in place.  st: dict(ids [B, S], ids_len, finished, emitted, pending, toks [B, max_new],
    lats [B, max_new, d], drop_target, drop_assistant, rounds, drafted, accepted, max_new); logits [B, k + 1, V]; latents
    [B, k + 1, d]; drafts [B, >= k] (None for k = 0)."""
    kw = kw or {}
    B = logits.shape[0]
    for b in range(B):
        len0, em0 = int(st["ids_len"][b]), int(st["emitted"][b])
        if st["finished"][b] or em0 >= st["max_new"]:
            st["finished"][b] = 1
            st["drop_target"][b] = st["drop_assistant"][b] = appended
            continue
        kk = min(k, st["max_new"] - em0 - 1) if drafts is not None else 0
        m = acc = 0
        fin = False
        for i in range(kk + 1):
            if i > 0:
                st["ids"][b, len0 + i - 1] = drafts[b, i - 1]
            row = [int(x) for x in st["ids"][b, :len0 + i]]
            tok, _ = chain_token(logits[b, i], row, plen, kw, rep, eos)
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
        st["ids_len"][b] = len0 + m
        st["emitted"][b] = em0 + m
        st["pending"][b] = last
        st["finished"][b] = 1 if fin or em0 + m >= st["max_new"] else 0
        st["drop_target"][b] = st["drop_assistant"][b] = appended - m if appended > 0 else 0
        if appended > 0:
            st["rounds"][b] += 1
            st["drafted"][b] += kk
            st["accepted"][b] += acc
    return st
