"""Plain torch restatements of what the attention kernels (csrc/gpt_kernels.h, csrc/attn64.h) compute, written from their comments:
softmax(scale * q k^T) v with a per-row key limit and a per-(batch, key) keep mask, the chunk partials of k_attention and their merge,
the GPT cache layout, and the fused attention + c_proj partials.  Every function works in the dtype of its inputs: fp64 for the
reference, fp32 for the restatement that measures what a correct fp32 evaluation deviates by.  tests/test_attn_oracle_host.py checks
them against torch.nn.functional.scaled_dot_product_attention; tests/test_gpu_attn_modes.py compares the kernels with them.

Rows that see no key: the masked tile kernels document zeros (linv = 0), so `empty="zero"` gives zeros; k_attn64_mfma divides 0 by 0
there (every wave's weight is 0, L = 0, 0 * (1 / 0)), as the softmax of a row of -inf does, so `empty="nan"` keeps torch's NaN."""
import torch

from gemm_oracle import fm16_index, fm16_perm      # noqa: F401  (the FM16 map is the GEMMs'; restated and checked there)

NEG_INF = float("-inf")


def scores(q, k, scale, limits, mask=None):
    """q [B][H][Tq][D], k [B][H][Tk][D], limits int [B][Tq], mask bool [B][Tk] (True = keep) -> (s [B][H][Tq][Tk] with -inf where
    the row does not see the key, visible bool [B][1][Tq][Tk])"""
    Tk = k.shape[2]
    vis = torch.arange(Tk).view(1, 1, Tk) < limits.unsqueeze(-1)
    if mask is not None:
        vis = vis & mask.bool().unsqueeze(1)
    vis = vis.unsqueeze(1)
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    return s.masked_fill(~vis, NEG_INF), vis


def attend(q, k, v, scale, limits, mask=None, empty="zero"):
    """softmax(scale * q k^T) v per (batch, head, row): -> [B][H][Tq][D].  Row (b, t) sees keys j < limits[b][t] with mask[b][j]"""
    s, vis = scores(q, k, scale, limits, mask)
    p = torch.softmax(s, dim=-1)                          # a row of -inf: NaN
    if empty == "zero":
        p = torch.where(vis.any(dim=-1, keepdim=True), p, torch.zeros_like(p))
    else:
        assert empty == "nan"
    return torch.matmul(p, v)


def partials(q, k, v, scale, limits, chunks):
    """k_attention's split of a row's nk = limits[b][t] keys: cs = ceil(nk / chunks), chunk c covers [c * cs, min(nk, (c + 1) * cs)).
    -> (o [B][H][Tq][chunks][D] = sum_j e^{s_j - m} v_j, m [B][H][Tq][chunks] = max_j s_j, l = sum_j e^{s_j - m}); an empty chunk is
    (0, -inf, 0)"""
    B, H, Tq, D = q.shape
    o = torch.zeros(B, H, Tq, chunks, D, dtype=q.dtype)
    m = torch.full((B, H, Tq, chunks), NEG_INF, dtype=q.dtype)
    l = torch.zeros(B, H, Tq, chunks, dtype=q.dtype)
    for b in range(B):
        for t in range(Tq):
            nk = int(limits[b, t])
            cs = -(-nk // chunks)
            for c in range(chunks):
                k0, k1 = c * cs, min(nk, (c + 1) * cs)
                if k1 <= k0:
                    continue
                s = torch.matmul(k[b, :, k0:k1], q[b, :, t].unsqueeze(-1)).squeeze(-1) * scale          # [H][n]
                mc = s.max(dim=-1).values
                p = torch.exp(s - mc.unsqueeze(-1))
                m[b, :, t, c] = mc
                l[b, :, t, c] = p.sum(dim=-1)
                o[b, :, t, c] = torch.matmul(p.unsqueeze(1), v[b, :, k0:k1]).squeeze(1)
    return o, m, l


def merge(o, m, l):
    """chunk partials -> the normalised row [B][H][Tq][D]: sum_c e^{m_c - M} o_c / sum_c e^{m_c - M} l_c (an empty chunk weighs 0)"""
    M = m.max(dim=-1, keepdim=True).values
    w = torch.where(m == NEG_INF, torch.zeros_like(m), torch.exp(m - M))
    return (w.unsqueeze(-1) * o).sum(dim=-2) / (w * l).sum(dim=-1, keepdim=True)


# ---- the GPT cache: [slot][head][max_seq][HD]; batch entry b lives in slot slots[b], whose first base_len[slot] rows were cached by
# earlier calls; row b * T + t of a causal call sees base_len[slot] + t + 1 keys ----
def causal_limits(slots, base_len, T):
    """-> int [B][T]; base_len None: no cached keys"""
    t = torch.arange(T).view(1, T)
    if base_len is None:
        return (t + 1).expand(len(slots), T).contiguous()
    return base_len[slots].view(-1, 1) + t + 1


def cache_keys(cache, slots):
    """cache [n_slots][H][max_seq][D] -> the batch's keys (or values) [B][H][max_seq][D]"""
    return cache[slots]


def bf16_cache(x):
    """fp32 -> the values a bf16 cache holds (round to nearest even, torch's conversion), widened back exactly"""
    return x.to(torch.bfloat16).to(torch.float32)


def fused_proj(att, Wp):
    """att [H][D] (the normalised row of every head), Wp [d][d] row-per-output with d = H * D -> part2 [H][d]:
    part2[h] = Wp[:, h * D:(h + 1) * D] @ att[h]; their sum over h is the projection"""
    H, D = att.shape
    return torch.stack([Wp[:, h * D:(h + 1) * D] @ att[h] for h in range(H)])
