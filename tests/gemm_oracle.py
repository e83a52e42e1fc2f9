"""fp64 CPU restatements of what csrc/gemm.h promises about the fp32 GEMM kernels, written from its comments: the FM16 index map,
the epilogue order, the implicit-conv operand gather, the attention-partial merge, LayerNorm after a row completion, and bf16
round-to-nearest-even.  tests/test_gemm_oracle_host.py checks each against torch's own functions; tests/test_gpu_gemm_modes.py
compares the kernels with them."""
import math

import torch

ACT_NONE, ACT_GELU_NEW, ACT_RELU, ACT_GELU_ERF = 0, 1, 2, 3
LN_EPS = 1e-5


# ---- FM16: each (16 rows x 16 k) block is 256 contiguous floats = 64 float4; float4 slot (m % 16) + 16 * ((k % 16) / 4) holds the four
# consecutive k of row m that start at a multiple of 4; blocks are ordered row-block major, k-block minor ----
def fm16_index(m, k, K):
    block = (m // 16) * (K // 16) + k // 16
    slot = m % 16 + 16 * ((k % 16) // 4)
    return block * 256 + slot * 4 + k % 4


def fm16_perm(M, K):
    """flat FM16 position of every (m, k) of an [M][K] matrix (M, K multiples of 16), as an int64 [M][K] tensor"""
    m = torch.arange(M).view(M, 1)
    k = torch.arange(K).view(1, K)
    return (m // 16 * (K // 16) + k // 16) * 256 + (m % 16 + 16 * (k % 16 // 4)) * 4 + k % 4


def to_fm16(x, pad_rows_to=16, fill=0.0):
    """row-major [M][K] -> flat FM16 of [Mp][K], Mp = M rounded up; the padding rows hold `fill`"""
    M, K = x.shape
    Mp = -(-M // pad_rows_to) * pad_rows_to
    xp = torch.full((Mp, K), fill, dtype=x.dtype)
    xp[:M] = x
    out = torch.empty(Mp * K, dtype=x.dtype)
    out[fm16_perm(Mp, K).reshape(-1)] = xp.reshape(-1)
    return out


def from_fm16(flat, M, K):
    """flat FM16 of [Mp][K] -> row-major [M][K]"""
    Mp = flat.numel() // K
    return flat[fm16_perm(Mp, K).reshape(-1)].view(Mp, K)[:M]


# ---- bf16 round to nearest, ties to even, on the bit pattern (finite inputs) ----
def bf16_bits(x):
    """uint16 patterns (as int32 tensor) of fp32 x rounded to bf16, nearest even"""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    lower = u & 0xFFFF
    up = (lower > 0x8000) | ((lower == 0x8000) & (((u >> 16) & 1) == 1))
    return (((u >> 16) + up.to(torch.int64)) & 0xFFFF).to(torch.int32)


def bf16_round(x):
    """fp32 x rounded to the nearest bf16 value (ties to even), returned as fp32"""
    b = bf16_bits(x).to(torch.int64) << 16
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    return b.to(torch.int32).view(torch.float32).view(x.shape)


# ---- activations ----
def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def activation(x, act):
    if act == ACT_GELU_NEW:
        return gelu_new(x)
    if act == ACT_RELU:
        return torch.clamp(x, min=0.0)
    if act == ACT_GELU_ERF:
        return gelu_erf(x)
    return x


def leaky_relu(x, slope):
    return torch.where(x > 0, x, x * slope)


# ---- epilogues.  `acc` is the [M][N] product; everything in the dtype of acc (fp64 for the reference, fp32 for the restatement
# that measures what a correct fp32 evaluation of the same formula deviates by) ----
def epilogue(acc, bias=None, act=ACT_NONE, resid=None, resid2=None, out_scale=0.0):
    """bias, then activation, then + resid, + resid2, then * out_scale (0 = none)"""
    v = acc if bias is None else acc + bias
    v = activation(v, act)
    if resid is not None:
        v = v + resid
    if resid2 is not None:
        v = v + resid2
    if out_scale != 0.0:
        v = v * out_scale
    return v


def geglu(acc, bias=None):
    """columns are (x_j, gate_j) pairs: column j of the [M][N / 2] result is gelu_erf(gate_j) * x_j"""
    v = acc if bias is None else acc + bias
    return gelu_erf(v[:, 1::2]) * v[:, 0::2]


def qkv_scatter(acc, bias, act, d, n_head, head_dim, T, slots, base_len, kcache, vcache):
    """columns [0, d) -> q [M][d] (returned); [d, 2d) / [2d, 3d) -> row t of batch entry b = m // T goes to
    cache[slots[b]][h][base_len[slots[b]] + t][j].  kcache / vcache [n_slots][n_head][max_seq][head_dim] are updated in place."""
    v = activation(acc if bias is None else acc + bias, act)
    M = v.shape[0]
    for m in range(M):
        b, t = divmod(m, T)
        slot = int(slots[b])
        pos = t + (int(base_len[slot]) if base_len is not None else 0)
        kcache[slot, :, pos, :] = v[m, d:2 * d].view(n_head, head_dim)
        vcache[slot, :, pos, :] = v[m, 2 * d:3 * d].view(n_head, head_dim)
    return v[:, :d].clone()


# ---- implicit im2col: column k of A is (tap = k // Ci, ci = k % Ci) and lives at buf[(m + tap * dil) rows down][ci] ----
def conv_gather(xpad, taps, dil, T):
    """xpad [rows][Ci] time-major, already offset so that output row m reads rows m + tap * dil: -> A [T][taps * Ci]"""
    return torch.cat([xpad[tap * dil: tap * dil + T] for tap in range(taps)], dim=1)


def conv_weight_matrix(w):
    """conv1d weight [Co][Ci][k] -> Wt [Co][k * Ci] in the (tap, ci) column order of conv_gather"""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1)


# ---- attention partials: per (row, head, chunk) a tuple (o[hd], m, l); merged row = sum_c e^{m_c - M} o_c / sum_c e^{m_c - M} l_c ----
def att_merge(part, hd):
    """part [M][heads][nc][hd + 4] -> A [M][heads * hd]"""
    o, m, l = part[..., :hd], part[..., hd], part[..., hd + 1]
    w = torch.exp(m - m.max(dim=-1, keepdim=True).values)
    out = (w.unsqueeze(-1) * o).sum(dim=2) / (w * l).sum(dim=-1, keepdim=True)
    return out.reshape(part.shape[0], -1)


# ---- row completion + LayerNorm ----
def row_complete(x, bias=None, part=None):
    """x + bias + part[0] + ... (bias and part only together with part, as the kernels take them)"""
    if part is None:
        return x.clone()
    v = x + bias
    for s in range(part.shape[0]):
        v = v + part[s]
    return v


def layer_norm(v, w, b, eps=LN_EPS):
    mean = v.mean(dim=-1, keepdim=True)
    var = ((v - mean) ** 2).mean(dim=-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * w + b


def row_stats(v, eps=LN_EPS):
    mean = v.mean(dim=-1)
    var = ((v - mean.unsqueeze(-1)) ** 2).mean(dim=-1)
    return mean, 1.0 / torch.sqrt(var + eps)


def gemm_tol(K, ref):
    """the project's bound for a plain fp32 GEMM against fp64 (tests/test_gpu_gemm.py)"""
    return 2e-5 * (K / 256) ** 0.5 * max(1.0, float(ref.abs().max()))
