"""Every attention kernel (csrc/gpt_kernels.h: k_attention, k_attn_proj, k_attention_tile, k_attention_tile_short; csrc/attn64.h:
k_attn64_mfma) alone, through the C-ABI test hook gvc_attn_probe on buffers this file owns, against the fp64 oracle tests/attn_oracle.py
(itself checked against torch's attention in tests/test_attn_oracle_host.py).

Rules of every case (those of tests/test_gpu_gemm_modes.py): inputs come from genvc_amd.synth with fixed seeds; every output is pre-filled
with a NaN bit pattern between two guard regions, every element the call owns must match the reference and every other element must keep
the pattern bit for bit; what the call must not read is NaN on the device -- cache rows at or past a stream's last visible key, slots the
call does not name, k_attn64_mfma rows at or past Tk, columns of other layers -- so a load that leaks (the kernels clamp theirs to the
last valid row) poisons the result.  Per-slot integers of slots the call does not name are valid but different, so a wrong index shows as
a wrong result, never as a wild address.

Score regimes (checked on the CPU from the oracle's scores alone, before anything runs): uniform (score deviation 0.5), peaked (8: the top
key holds most of the mass), offset (every score near +60: the maximum subtraction) and ordered (last key largest, first key second, the
rest ascending by 0.25 per key: every new tile, chunk, wave or lane group raises its running maximum -- the alpha rescale); for the
fused kernel also late (keys 64.. more than 95 above keys 0..63: a maximum over half the score slots overflows).

Bounds, from the case's own inputs on the CPU, never from the kernel: e32 = max |plain fp32 torch evaluation - fp64 oracle|.
  GPT kernels (__expf):  4 * e32 + 6e-6 * max|V|  (argument scaling of __expf costs |x| * 2^-24 relative; terms with x < -17 carry less
                         than 4e-8 of the mass; together about 2.3e-6 relative on a weight; 4x for the MFMA / wave summation order);
  k_attn64_mfma (expf):  4 * e32 + 2^-22 * max|ref|;
  a chunk maximum m:     4 * e32(m) + 2^-22 * max|m| (a plain fp32 dot product: summation order, and a floor of four ulps);
  producer -> skinny GEMM consumer: the larger of the GEMM modes' bound and 4 * e32 of the fp32 restatement of attend @ W^T; and, through
                         a selection matrix (exact), the attention bound itself on the consumer's merged rows.
DESIGN.md "Attention mode tests" records the matrix, the instantiations and the measured figures (printed with pytest -s)."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as AO                      # noqa: E402
import gemm_oracle as GO                      # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAT = 0x7FC0BEEF            # a quiet NaN nobody computes
PAT16 = 0x7FC07FC0          # two bf16 quiet NaNs
GUARD = 256                 # 4-byte elements on each side
NAN = float("nan")
ROWS, TILE, TILE_MASKED, FUSED_PROJ, ATTN64 = range(5)
RAN_NONE, RAN_SHORT, RAN_TILED = range(3)
REGIMES = ("uniform", "peaked", "offset", "ordered")
STEP = 0.25                 # score step of the ordered regime
H = 2                       # heads of the GPT-kernel cases (the head index is a grid dimension: two show a wrong stride)
STATS = {}                  # family -> [max e32, max error, max error / bound, cases]


class Buf:
    """n 4-byte elements on the device between two guard regions; payload = `data` (fp32 / int32 CPU tensor) or the NaN pattern"""

    def __init__(self, n=None, data=None, pat=PAT):
        if data is not None:
            data = data.contiguous().reshape(-1)
            n = data.numel()
        self.n, self.pat = n, pat
        self.raw = torch.full((n + 2 * GUARD,), pat, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + n]
        if data is not None:
            self.t.copy_(data.view(torch.int32))

    def ptr(self, off=0):
        return self.t.data_ptr() + 4 * off

    def bits(self):
        return self.t.cpu()

    def guards_ok(self):
        raw = self.raw.cpu()
        return bool((raw[:GUARD] == self.pat).all()) and bool((raw[GUARD + self.n:] == self.pat).all())


def kv_buf(x, kvb):
    """a K or V cache (fp32 CPU tensor, NaN where the call must not read) as the device stores it: fp32, or bf16 pairs"""
    if not kvb:
        return Buf(data=x)
    return Buf(data=x.to(torch.bfloat16).contiguous().view(torch.int16).reshape(-1).view(torch.int32), pat=PAT16)


def probe(kind, **kw):
    """one gvc_attn_probe call; Buf arguments become their payload address.  -> (rc, case)"""
    from genvc_amd import _lib
    c = _lib.AttnCase()
    c.kind = kind
    for k, v in kw.items():
        setattr(c, k, v.ptr() if isinstance(v, Buf) else v)
    return _lib.lib().gvc_attn_probe(C.byref(c), _lib.stream()), c


def ok(kind, **kw):
    rc, c = probe(kind, **kw)
    if rc != 0:
        from genvc_amd import _lib
        raise AssertionError(f"attn probe kind {kind} failed with {rc}: {_lib.lib().gvc_last_error().decode()}")
    return c


def gemm_ok(kind, **kw):
    from genvc_amd import _lib
    c = _lib.GemmCase()
    c.kind = kind
    for k, v in kw.items():
        setattr(c, k, v.ptr() if isinstance(v, Buf) else v)
    rc = _lib.lib().gvc_gemm_probe_ex(C.byref(c), _lib.stream())
    assert rc == 0, (kind, rc, _lib.lib().gvc_last_error().decode())


def out_idx(rows, d, fm16):
    """(buffer elements, flat positions of the [rows][d] result in (row, column) order)"""
    if fm16:
        Mp = -(-rows // 16) * 16
        return Mp * d, GO.fm16_perm(Mp, d)[:rows].reshape(-1)
    return rows * d, torch.arange(rows * d)


def check(buf, idx, ref, tol, what):
    """buf[idx] matches ref (fp64, same order) within tol; every other element and both guards still hold the pattern"""
    bits = buf.bits()
    owned = torch.zeros(buf.n, dtype=torch.bool)
    owned[idx] = True
    assert int(owned.sum()) == idx.numel(), what
    assert bool((bits[~owned] == PAT).all()), (what, "an element outside the result was written", int((bits[~owned] != PAT).sum()))
    assert buf.guards_ok(), (what, "guard region written")
    out = bits.view(torch.float32)[idx].double()
    assert bool(torch.isfinite(out).all()), (what, "non-finite result", int((~torch.isfinite(out)).sum()))
    err = float((out - ref.reshape(-1)).abs().max())
    assert err < tol, (what, err, tol)
    return err


def note(family, e32, err, tol):
    s = STATS.setdefault(family, [0.0, 0.0, 0.0, 0])
    s[0], s[1], s[2], s[3] = max(s[0], e32), max(s[1], err), max(s[2], err / tol), s[3] + 1


def gpt_tol(e32, v):
    return 4.0 * e32 + 6e-6 * float(v.abs().max())


def a64_tol(e32, ref):
    return 4.0 * e32 + 2.0 ** -22 * float(ref.abs().max())


# ------------------------------------------------------------------ inputs ------------------------------------------------------------------
def basis(seed, D):
    """sign vectors on disjoint dimensions (no product of two ever cancels): u1 on d % 4 == 0, u3 on d % 4 == 1, u2 on the rest; r on all"""
    r = torch.where(synth.uniform(seed, "signs", (D,)) < 0, -1.0, 1.0)
    i = torch.arange(D)
    return r * (i % 4 == 0), r * (i % 4 >= 2), r * (i % 4 == 1), r


def make_inputs(seed, regime, D, heads, B, T, n_slots, max_seq, scale, limits, kvb=0):
    """q [B][T][heads][D], K and V caches [n_slots][heads][max_seq][D] (finite everywhere; bf16-representable with kvb) of a regime.
    limits [B][T]: the keys each row sees (the ordered regime places the first key's score from it)."""
    q = synth.uniform(seed, "q", (B, T, heads, D))
    kc = synth.uniform(seed, "k", (n_slots, heads, max_seq, D))
    vc = synth.uniform(seed, "v", (n_slots, heads, max_seq, D))
    u1, u2, u3, r = basis(seed, D)
    if regime == "uniform":
        q = q * (0.5 / (scale * math.sqrt(D)))
    elif regime == "peaked":
        q = q * (8.0 / (scale * math.sqrt(D)))
    elif regime == "offset":        # one common component a e (|e| = 1) in q and k: scale * a^2 = 60 on every score
        a = math.sqrt(60.0 / scale)
        q = q * (0.5 / (scale * math.sqrt(D))) + a * r / math.sqrt(D)
        kc = kc + a * r / math.sqrt(D)
    elif regime == "late":          # (the fused kernel's case) keys from 64 on score about 120 above the earlier ones
        a = math.sqrt(120.0 / scale)
        q = q * (0.5 / (scale * math.sqrt(D))) + a * r / math.sqrt(D)
        kc[:, :, 64:] += a * r / math.sqrt(D)
    else:                           # ordered: key j >= 1 scores STEP * j, key 0 scores STEP * (nk - 1.5) for a row of nk keys
        j = torch.arange(max_seq)
        hi, lo = (j // 16 * 16).float().view(-1, 1), (j % 16).float().view(-1, 1)          # each exact in bf16
        noise = kc * 0.001
        kc = hi * u1 + lo * u3 + noise
        kc[:, :, 0] = u2 + noise[:, :, 0]
        beta = STEP * (limits.float() - 1.5) / (scale * D / 2)                               # |u2|^2 = D / 2, |u1|^2 = |u3|^2 = D / 4
        q = (STEP / (scale * D / 4)) * (u1 + u3).expand(B, T, heads, D) + beta.view(B, T, 1, 1) * u2
    if kvb:
        kc, vc = AO.bf16_cache(kc), AO.bf16_cache(vc)
    return q.contiguous(), kc.contiguous(), vc.contiguous()


def check_regime(regime, q, k, scale, limits, what):
    """the regime is what it claims, from the oracle's fp64 scores (no mask)"""
    s, vis = AO.scores(q.double(), k.double(), scale, limits)
    n = limits.view(limits.shape[0], 1, -1).expand(s.shape[:3])             # [B][H][Tq]
    p = torch.softmax(s, dim=-1)
    top = p.max(dim=-1).values
    if regime == "uniform":
        assert bool((top[n >= 8] < 0.5).all()), what
    elif regime == "peaked":
        big = n >= 8
        if bool(big.any()):
            sd = float(s[vis.expand_as(s) & big.unsqueeze(-1)].std())
            assert 6.0 < sd < 10.0, (what, "score deviation about 8", sd)
            if int(big.sum()) >= 24:
                assert float((top[big] > 0.5).double().mean()) > 0.5, (what, "the top key holds more than half the mass for most rows")
            else:           # a handful of rows: their mean instead of a count
                assert float(top[big].mean()) > 0.4, (what, "the top key holds most of the mass", float(top[big].mean()))
    elif regime == "offset":
        sv = s[vis.expand_as(s)]
        assert float(sv.min()) > 40.0 and float(sv.max()) < 80.0, (what, float(sv.min()), float(sv.max()))
    elif regime == "late":
        assert bool((n > 64).all()) and float(s[..., 64:][vis.expand_as(s)[..., 64:]].min()) - float(s[..., :64].max()) > 95.0, what
    else:
        Tk = s.shape[-1]
        idx = torch.arange(Tk - 1).view(1, 1, 1, -1)
        pair = (idx >= 1) & (idx + 1 < n.unsqueeze(-1))                      # (j, j + 1), both seen, j >= 1
        dlt = s[..., 1:] - s[..., :-1]
        assert bool((dlt[pair] > 0.5 * STEP).all()), (what, "scores ascend with the key index")
        assert bool((s.argmax(dim=-1) == n - 1).all()), (what, "the last key is the row's maximum")
        last = s.gather(-1, (n - 1).clamp(min=0).unsqueeze(-1)).squeeze(-1)
        prev = s.gather(-1, (n - 2).clamp(min=0).unsqueeze(-1)).squeeze(-1)
        three = n >= 3
        assert bool((s[..., 0][three] < last[three]).all()) and bool((s[..., 0][three] > prev[three]).all()), (what, "the first key is second")


def poisoned(cache, slots, n_vis):
    """NaN everywhere except the first n_vis[b] rows of slot slots[b]"""
    c = torch.full_like(cache, NAN)
    for b, slot in enumerate(slots.tolist()):
        c[slot, :, :n_vis[b]] = cache[slot, :, :n_vis[b]]
    return c


class GptCase:
    """one call of a GPT attention kernel on the cache layout [slot][head][max_seq][D]: inputs, device buffers, oracle results"""

    def __init__(self, seed, regime, D, kvb, B, T, slots, base, n_slots, max_seq, causal=1, n_keys=0, mask=None, heads=H):
        self.D, self.kvb, self.B, self.T, self.heads, self.max_seq, self.n_slots = D, kvb, B, T, heads, max_seq, n_slots
        self.scale = 1.0 / math.sqrt(D)
        self.slots, self.base = torch.tensor(slots), (None if base is None else torch.tensor(base))
        self.limits = AO.causal_limits(self.slots, self.base, T) if causal else torch.full((B, T), n_keys)
        assert int(self.limits.max()) <= max_seq
        q, kc, vc = make_inputs(seed, regime, D, heads, B, T, n_slots, max_seq, self.scale, self.limits, kvb)
        if mask is not None:            # keep flags of the first keys; the cache rows past them are past every row's limit
            mask = torch.cat([mask, torch.ones(B, max_seq - mask.shape[1], dtype=torch.bool)], dim=1)
        self.q, self.mask = q, mask
        self.qh = q.permute(0, 2, 1, 3)                                        # [B][H][T][D]
        self.k, self.v = AO.cache_keys(kc, self.slots), AO.cache_keys(vc, self.slots)
        if mask is None:
            check_regime(regime, self.qh, self.k, self.scale, self.limits, (regime, D, kvb, B, T))
        n_vis = self.limits.max(dim=1).values.tolist()
        self.kd, self.vd = kv_buf(poisoned(kc, self.slots, n_vis), kvb), kv_buf(poisoned(vc, self.slots, n_vis), kvb)
        self.qd = Buf(data=q)
        self.slots_d = Buf(data=self.slots.to(torch.int32))
        self.base_d = None if self.base is None else Buf(data=self.base.to(torch.int32))
        self.ref = AO.attend(self.qh.double(), self.k.double(), self.v.double(), self.scale, self.limits, mask)
        r32 = AO.attend(self.qh, self.k, self.v, self.scale, self.limits, mask)
        self.e32 = float((r32.double() - self.ref).abs().max())
        self.tol = gpt_tol(self.e32, self.v)
        self.args = dict(head_dim=D, n_head=heads, kv_bf16=kvb, q=self.qd, q_stride=heads * D, kbase=self.kd, vbase=self.vd,
                         k_batch_stride=heads * max_seq * D, k_head_stride=max_seq * D, k_row_stride=D, T=T, slots=self.slots_d,
                         base_len=self.base_d, causal=causal, n_keys=n_keys, scale=self.scale, out_stride=heads * D)

    def rows_ref(self, x=None):
        """[B][H][T][D] -> [B * T][H * D], the kernels' output rows"""
        x = self.ref if x is None else x
        return x.permute(0, 2, 1, 3).reshape(self.B * self.T, self.heads * self.D)

    def run_direct(self, kind, fm16, family, what, **extra):
        rows, d = self.B * self.T, self.heads * self.D
        n, idx = out_idx(rows, d, fm16)
        out = Buf(n)
        c = ok(kind, out=out, out_fm16=fm16, **dict(self.args, **extra))
        if kind != ROWS and not c.taken:
            return c, out, None
        err = check(out, idx, self.rows_ref(), self.tol, what)
        note(family, self.e32, err, self.tol)
        return c, out, err


def mixed_base(n_slots, slots, bases, other=1):
    """per-slot base_len: the named slots get `bases`, every other slot a valid length of its own"""
    b = [other] * n_slots
    for s, v in zip(slots, bases):
        b[s] = v
    return b


# ------------------------------------------------------------------ k_attention, direct ------------------------------------------------------------------
ROWS_CFG = [(256, 0, 0), (256, 1, 0), (128, 0, 0), (128, 1, 0), (64, 0, 0), (64, 1, 0), (256, 0, 1), (256, 1, 1)]       # (HD, bf16 cache, wide)
# key counts around one pass of the kernel's loop (U * NW * KPW keys: 16, 32, 64; wide 128)
ROWS_COUNTS = {(256, 0): (1, 15, 16, 17, 33), (128, 0): (1, 31, 32, 33, 70), (64, 0): (1, 63, 64, 65, 130), (256, 1): (1, 127, 128, 129, 300)}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("D,kvb,wide", ROWS_CFG)
def test_rows_direct(D, kvb, wide, regime):
    cnt = ROWS_COUNTS[(D, wide)]
    max_seq = cnt[-1] + 4
    seed = 1000 + D + 7 * kvb + 13 * wide
    worst = 0.0
    for fm16 in (0, 1):
        # T = 1 over three streams in slots [2, 0, 3] of five, each with its own cached length
        for trio in (cnt[0:3], cnt[2:5]):
            slots = [2, 0, 3]
            g = GptCase(seed, regime, D, kvb, 3, 1, slots, mixed_base(5, slots, [n - 1 for n in trio]), 5, max_seq)
            assert g.limits.view(-1).tolist() == list(trio)
            worst = max(worst, g.run_direct(ROWS, fm16, "k_attention direct", ("rows direct", D, kvb, wide, regime, trio, fm16), chunks=1, rows=3,
                                            direct=1, wide=wide)[2] / g.tol)
        # the verify shape: T = 3 behind a base, the three rows straddle the loop's pass boundary (and its multiple)
        slots = [3, 1]
        g = GptCase(seed + 1, regime, D, kvb, 2, 3, slots, mixed_base(5, slots, [cnt[2] - 2, cnt[4] - 3]), 5, max_seq)
        assert g.limits.tolist() == [[cnt[2] - 1, cnt[2], cnt[2] + 1], [cnt[4] - 2, cnt[4] - 1, cnt[4]]]
        worst = max(worst, g.run_direct(ROWS, fm16, "k_attention direct", ("rows verify", D, kvb, wide, regime, fm16), chunks=1, rows=6, direct=1,
                                        wide=wide)[2] / g.tol)
    print(f"[attn-modes] k_attention<{D}, direct, NW {16 if wide else 4}, KVB {kvb}> {regime}: worst err / bound {worst:.3f}")


# ------------------------------------------------------------------ k_attention, chunk partials ------------------------------------------------------------------
def run_partials(g, chunks, wide, what):
    """-> (out Buf, kernel partials as fp64 (o, m, l) in the oracle's [B][H][T][chunks] order); checks ownership, every triple, the merge"""
    D, rows = g.D, g.B * g.T
    tup = D + 4
    out = Buf(rows * g.heads * chunks * tup)
    ok(ROWS, out=out, chunks=chunks, rows=rows, direct=0, wide=wide, **g.args)
    bits = out.bits()
    raw = bits.view(rows * g.heads * chunks, tup)
    assert bool((raw[:, D + 2:] == PAT).all()), (what, "the tuple's padding was written")
    assert out.guards_ok(), (what, "guard region written")
    part = raw.view(torch.float32).double().view(g.B, g.T, g.heads, chunks, tup).permute(0, 2, 1, 3, 4)
    o, m, l = part[..., :D], part[..., D], part[..., D + 1]
    o64, m64, l64 = AO.partials(g.qh.double(), g.k.double(), g.v.double(), g.scale, g.limits, chunks)
    o32, m32, l32 = AO.partials(g.qh, g.k, g.v, g.scale, g.limits, chunks)
    empty = l64 == 0
    assert bool((o[empty] == 0).all()) and bool((m[empty] == AO.NEG_INF).all()) and bool((l[empty] == 0).all()), (what, "an empty chunk is (0, -inf, 0)")
    full = ~empty
    assert bool(torch.isfinite(o[full]).all()) and bool(torch.isfinite(m[full]).all()) and bool((l[full] > 0).all()), (what, "non-finite partial")
    # each triple through its meaning: the chunk's own attention o / l, and its maximum
    n64 = o64[full] / l64[full].unsqueeze(-1)
    e32o = float(((o32[full] / l32[full].unsqueeze(-1)).double() - n64).abs().max())
    err_o = float((o[full] / l[full].unsqueeze(-1) - n64).abs().max())
    assert err_o < gpt_tol(e32o, g.v), (what, "o / l of a chunk", err_o, gpt_tol(e32o, g.v))
    e32m = float((m32[full].double() - m64[full]).abs().max())
    tol_m = 4.0 * e32m + 2.0 ** -22 * float(m64[full].abs().max())
    err_m = float((m[full] - m64[full]).abs().max())
    assert err_m < tol_m, (what, "m of a chunk", err_m, tol_m)
    err = float((AO.merge(o, m, l) - g.ref).abs().max())
    assert err < g.tol, (what, "merged partials", err, g.tol)
    note("k_attention partials", max(g.e32, e32o), max(err, err_o), g.tol)
    return out, err / g.tol


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("D,kvb,wide", ROWS_CFG)
def test_rows_partials(D, kvb, wide, regime):
    seed = 2000 + D + 7 * kvb + 13 * wide
    slots, worst = [2, 0, 3], 0.0
    for chunks in (2, 4, 8):
        # 3 keys: empty chunks with 4 and 8; 31 / 33 / 63 / 65: either side of a multiple of every chunk count; 130: several loop passes
        for trio in ((3, 31, 33), (65, 130, 63)):
            g = GptCase(seed + chunks, regime, D, kvb, 3, 1, slots, mixed_base(5, slots, [n - 1 for n in trio]), 5, 134)
            worst = max(worst, run_partials(g, chunks, wide, ("partials", D, kvb, wide, regime, chunks, trio))[1])
    print(f"[attn-modes] k_attention<{D}, partials, NW {16 if wide else 4}, KVB {kvb}> {regime}: worst merged err / bound {worst:.3f}")


@pytest.mark.parametrize("M", [9, 25])
@pytest.mark.parametrize("chunks", [2, 4])
def test_partials_feed_the_skinny_gemm(M, chunks):
    """producer to consumer: the wide kernel's own partials as the att_part operand of the skinny GEMM (the batched decode's c_proj)"""
    D, N = 256, 48
    K = H * D
    slots = [(5 * i + 3) % (M + 2) for i in range(M)]                          # a permutation of M of the M + 2 slots
    assert len(set(slots)) == M
    bases = synth.integers(31 + M, "bases", (M,), 150).tolist()
    bases[0], bases[1] = 2, 127                                                # fewer keys than chunks; one short of the wide loop's pass
    g = GptCase(3000 + M + chunks, "peaked", D, 0, M, 1, slots, mixed_base(M + 2, slots, bases), M + 2, 152)
    part, _ = run_partials(g, chunks, 1, ("partials for the GEMM", M, chunks))
    W, b = synth.uniform(77, "W", (N, K), 0.1), synth.uniform(77, "b", (N,))
    wsrc, wfm = Buf(data=W), Buf(N * K)
    gemm_ok(7, A=wsrc, C=wfm, M=N, K=K)                                        # GVC_GEMM_TO_FM16
    out = Buf(M * N)
    gemm_ok(1, att_part=part, att_nc=chunks, att_heads=H, att_hd=D, W=wfm, C=out, bias=Buf(data=b), M=M, N=N, K=K, lda=K, ldw=K, ldc=N, sk=1)
    ref = g.rows_ref() @ W.double().T + b.double()
    r32 = g.rows_ref(AO.attend(g.qh, g.k, g.v, g.scale, g.limits)) @ W.T + b
    e32 = float((r32.double() - ref).abs().max())
    tol = max(GO.gemm_tol(K, ref), 4.0 * e32)
    err = check(out, torch.arange(M * N), ref, tol, ("partials through the skinny GEMM", M, chunks))
    note("k_attention partials -> skinny GEMM", e32, err, tol)
    # the consumer's merge alone: a selection matrix (one 1.0 per row; products and sums with zeros are exact) hands 48 columns of the
    # merged rows through unchanged, so they are held to the attention bound itself, not to the looser bound of a product
    cols = (torch.arange(N) * 43 + 7) % K                                      # distinct, both heads
    Wsel = torch.zeros(N, K)
    Wsel[torch.arange(N), cols] = 1.0
    sfm, sel = Buf(N * K), Buf(M * N)
    gemm_ok(7, A=Buf(data=Wsel), C=sfm, M=N, K=K)
    gemm_ok(1, att_part=part, att_nc=chunks, att_heads=H, att_hd=D, W=sfm, C=sel, bias=Buf(data=torch.zeros(N)), M=M, N=N, K=K, lda=K, ldw=K, ldc=N,
            sk=1)
    err = check(sel, torch.arange(M * N), g.rows_ref()[:, cols], g.tol, ("merged rows through a selection matrix", M, chunks))
    note("skinny GEMM's merge of the partials", g.e32, err, g.tol)


# ------------------------------------------------------------------ tile kernels ------------------------------------------------------------------
TILE_CFG = [(256, 0), (256, 1), (128, 0), (128, 1), (64, 0), (64, 1)]
# name -> (B, T, slots, per-named-slot base or None, n_slots, max_seq, kernel)
TILE_CASES = {
    "short T17": (12, 17, [(7 * i + 2) % 13 for i in range(12)], None, 13, 20, RAN_SHORT),
    "short T100": (2, 100, [1, 0], None, 3, 104, RAN_SHORT),
    "short cached": (6, 20, [4, 0, 6, 2, 5, 1], [0, 5, 77, 77, 0, 5], 7, 128, RAN_SHORT),
    # 16 rows behind a base: the tile's key count base + 16 sits on the 64-key V-chunk boundaries 129 / 191 / 192 / 193 / 260
    "tiled cached T16": (12, 16, [(5 * i + 1) % 13 for i in range(12)], [113, 175, 176, 177, 244, 256, 112, 130, 0, 48, 64, 200], 13, 272, RAN_TILED),
    # 31 rows: the second tile (15 rows) sees base + 31 keys
    "tiled cached T31": (12, 31, [(5 * i + 1) % 13 for i in range(12)], [98, 160, 161, 162, 229, 241, 97, 100, 0, 33, 64, 128], 13, 272, RAN_TILED),
    "tiled T130": (2, 130, [1, 0], None, 3, 132, RAN_TILED),
}


def tile_case(name, seed, regime, D, kvb, **kw):
    B, T, slots, bases, n_slots, max_seq, ran = TILE_CASES[name]
    base = None if bases is None else mixed_base(n_slots, slots, bases)
    g = GptCase(seed, regime, D, kvb, B, T, slots, base, n_slots, max_seq, **kw)
    return g, ran


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("D,kvb", TILE_CFG)
def test_tile(D, kvb, regime):
    worst = {RAN_SHORT: 0.0, RAN_TILED: 0.0}
    for i, name in enumerate(TILE_CASES):
        g, ran = tile_case(name, 4000 + D + 7 * kvb + i, regime, D, kvb)
        max_keys = int(g.limits.max())
        assert (max_keys <= 128) == (ran == RAN_SHORT)
        if name == "tiled cached T16":
            assert {129, 191, 192, 193, 260} <= set(g.limits[:, -1].tolist())
        for fm16 in (0, 1):
            fam = "k_attention_tile_short" if ran == RAN_SHORT else "k_attention_tile"
            c, _, err = g.run_direct(TILE, fm16, fam, ("tile", name, D, kvb, regime, fm16), batch=g.B, max_keys=max_keys)
            assert c.taken == 1 and c.ran == ran, (name, c.taken, c.ran)
            worst[ran] = max(worst[ran], err / g.tol)
    print(f"[attn-modes] tile kernels HD {D} KVB {kvb} {regime}: worst err / bound short {worst[RAN_SHORT]:.3f}, tiled {worst[RAN_TILED]:.3f}")


def test_tile_chooser_declines_few_rows_and_few_tiles():
    for B, T in ((12, 15), (11, 16), (5, 32), (1, 100)):
        slots = list(range(B))
        g = GptCase(4500 + B, "uniform", 64, 0, B, T, slots, None, B, T + 4)
        c, out, _ = g.run_direct(TILE, 0, "none", ("declined", B, T), batch=B, max_keys=T)
        assert c.taken == 0 and c.ran == RAN_NONE, (B, T)
        assert bool((out.bits() == PAT).all()) and out.guards_ok()
    g = GptCase(4600, "uniform", 64, 0, 12, 16, list(range(12)), None, 12, 20)
    c, _, _ = g.run_direct(TILE, 0, "k_attention_tile_short", ("smallest taken", 12, 16), batch=12, max_keys=16)
    assert c.taken == 1 and c.ran == RAN_SHORT


# ------------------------------------------------------------------ non-causal AttnArgs ------------------------------------------------------------------
def test_non_causal_rows_and_tiles():
    """causal = 0: every row sees keys [0, n_keys) whatever base_len says; no product caller is left, the branch lives in three kernels"""
    for regime in REGIMES:
        slots = [2, 0, 3]
        g = GptCase(5000, regime, 128, 0, 3, 2, slots, mixed_base(5, slots, [9, 30, 2]), 5, 48, causal=0, n_keys=45)
        g.run_direct(ROWS, 0, "non-causal", ("rows non-causal", regime), chunks=1, rows=6, direct=1, wide=0)
        for n_keys, ran in ((100, RAN_SHORT), (150, RAN_TILED)):
            slots = [(5 * i + 1) % 13 for i in range(12)]
            g = GptCase(5001 + n_keys, regime, 128, 1, 12, 17, slots, mixed_base(13, slots, [3] * 12, other=7), 13, n_keys + 2, causal=0, n_keys=n_keys)
            c, _, _ = g.run_direct(TILE, 1, "non-causal", ("tile non-causal", regime, n_keys), batch=12, max_keys=n_keys)
            assert c.taken == 1 and c.ran == ran


# ------------------------------------------------------------------ masked tile kernels ------------------------------------------------------------------
def key_masks(B, T):
    """name -> keep flags [B][T] (True = attend)"""
    ones = torch.ones(B, T, dtype=torch.bool)
    first, tile, tail, alt, dead = ones.clone(), ones.clone(), ones.clone(), ones.clone(), ones.clone()
    first[:, 0] = False                                     # row 0 of every stream then sees nothing
    lo = 16 if T > 32 else 0
    tile[:, lo:lo + 16] = False                             # a whole 16-key tile
    for b in range(B):
        tail[b, T - 1 - 3 * b - (T // 3) * (b % 2):] = False       # padding tails of different lengths
    alt[:, 1::2] = False
    alt[-1, 0::2], alt[-1, 1::2] = False, True
    dead[0] = False                                         # one stream with every key masked
    return {"first key": first, "one tile": tile, "padding tail": tail, "alternating": alt, "dead stream": dead}


@pytest.mark.parametrize("T,B,ran", [(17, 12, RAN_SHORT), (100, 2, RAN_SHORT), (130, 2, RAN_TILED)])
@pytest.mark.parametrize("D", [256, 128, 64])
def test_tile_masked(D, T, B, ran):
    stride = T + 5
    slots = [(5 * i + 1) % (B + 1) for i in range(B)]
    fam = "k_attention_tile_short<MASK>" if ran == RAN_SHORT else "k_attention_tile<MASK>"

    def mask_buf(keep):
        m = torch.full((B, stride), 0x5A, dtype=torch.uint8)          # past T: never read (nonzero: a row that read it would attend)
        m[:, :T] = keep.to(torch.uint8)
        pad = (-m.numel()) % 4
        flat = torch.cat([m.reshape(-1), torch.zeros(pad, dtype=torch.uint8)])
        return Buf(data=flat.view(torch.int32))

    for regime in REGIMES:
        # an all-ones mask: the bits of the unmasked kernel
        g = GptCase(6000 + D + T, regime, D, 0, B, T, slots, None, B + 1, T + 3)
        c0, plain, _ = g.run_direct(TILE, 0, fam.replace("<MASK>", ""), ("unmasked twin", D, T, regime), batch=B, max_keys=T)
        assert c0.taken == 1 and c0.ran == ran
        c1, ones, _ = g.run_direct(TILE_MASKED, 0, fam, ("all-ones mask", D, T, regime), batch=B, max_keys=T,
                                   key_mask=mask_buf(torch.ones(B, T, dtype=torch.bool)), mask_stride=stride)
        assert c1.ran == ran and torch.equal(ones.bits(), plain.bits()), ("an all-ones mask changes the bits", D, T, regime)
        for name, keep in key_masks(B, T).items():
            for fm16 in (0, 1):
                gm = GptCase(6000 + D + T, regime, D, 0, B, T, slots, None, B + 1, T + 3, mask=keep)
                c, out, _ = gm.run_direct(TILE_MASKED, fm16, fam, ("masked", name, D, T, regime, fm16), batch=B, max_keys=T,
                                          key_mask=mask_buf(keep), mask_stride=stride)
                assert c.ran == ran
                # rows that see nothing are exact zeros
                seen = (keep.unsqueeze(1) & (torch.arange(T).view(1, 1, T) < gm.limits.unsqueeze(-1))).any(dim=-1)          # [B][T]
                if not bool(seen.all()):
                    n, idx = out_idx(B * T, H * D, fm16)
                    got = out.bits()[idx].view(B * T, H * D)
                    assert bool((got[~seen.view(-1)] == 0).all()), ("a row without a visible key is exact zeros", name, D, T)
                assert name not in ("first key", "dead stream") or not bool(seen.all())


# ------------------------------------------------------------------ fused attention + c_proj ------------------------------------------------------------------
_WP = {}


def wp(d):
    if d not in _WP:
        _WP[d] = synth.uniform(70 + d, "attn.c_proj", (d, d), 0.02)
    return _WP[d]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("d,kvb", [(512, 0), (512, 1), (1024, 0), (1024, 1)])
def test_fused_proj(d, kvb, regime):
    D, heads, n_slots, slot, max_seq = 256, d // 256, 4, 2, 132
    Wp = wp(d)
    wd = Buf(data=Wp)
    worst = 0.0
    for nk in (1, 7, 8, 9, 64, 127, 128):
        g = GptCase(7000 + d + nk, regime, D, kvb, 1, 1, [slot], mixed_base(n_slots, [slot], [nk - 1], other=3), n_slots, max_seq, heads=heads)
        ref = AO.fused_proj(g.ref[0, :, 0].double(), Wp.double())
        r32 = AO.fused_proj(AO.attend(g.qh, g.k, g.v, g.scale, g.limits)[0, :, 0], Wp)
        e32 = float((r32.double() - ref).abs().max())
        tol = gpt_tol(e32, g.v)
        out = Buf(heads * d)
        ok(FUSED_PROJ, head_dim=D, n_head=heads, kv_bf16=kvb, q=g.qd, kbase=g.kd, vbase=g.vd, slots=g.slots_d, seq_len=g.base_d, max_seq=max_seq,
           d=d, scale=g.scale, Wp=wd, out=out)
        err = check(out, torch.arange(heads * d), ref, tol, ("fused", d, kvb, regime, nk))
        note("k_attn_proj", e32, err, tol)
        worst = max(worst, err / tol)
    assert wd.guards_ok()
    print(f"[attn-modes] k_attn_proj<256, {kvb}> d {d} {regime}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("d,kvb", [(512, 0), (1024, 1)])
def test_fused_proj_maximum_among_the_late_keys(d, kvb):
    """the row maximum is taken over all 128 score slots: keys 64.. sit more than 95 above keys 0..63, so a maximum over the first 64 alone
    leaves e^95 (inf in fp32) where the regimes above, whose first key is never far below the maximum, would still normalise it away"""
    D, heads, n_slots, slot, max_seq = 256, d // 256, 4, 2, 132
    Wp = wp(d)
    for nk in (65, 100, 128):
        g = GptCase(7200 + d + nk, "late", D, kvb, 1, 1, [slot], mixed_base(n_slots, [slot], [nk - 1], other=3), n_slots, max_seq, heads=heads)
        ref = AO.fused_proj(g.ref[0, :, 0].double(), Wp.double())
        r32 = AO.fused_proj(AO.attend(g.qh, g.k, g.v, g.scale, g.limits)[0, :, 0], Wp)
        e32 = float((r32.double() - ref).abs().max())
        out = Buf(heads * d)
        ok(FUSED_PROJ, head_dim=D, n_head=heads, kv_bf16=kvb, q=g.qd, kbase=g.kd, vbase=g.vd, slots=g.slots_d, seq_len=g.base_d, max_seq=max_seq,
           d=d, scale=g.scale, Wp=Buf(data=Wp), out=out)
        err = check(out, torch.arange(heads * d), ref, gpt_tol(e32, g.v), ("fused, late maximum", d, kvb, nk))
        note("k_attn_proj", e32, err, gpt_tol(e32, g.v))


def test_fused_proj_refuses_what_the_kernel_cannot_hold():
    d, D, heads, n_slots, slot, max_seq = 512, 256, 2, 4, 2, 132
    g = GptCase(7100, "uniform", D, 0, 1, 1, [slot], mixed_base(n_slots, [slot], [128], other=3), n_slots, max_seq, heads=heads)      # 129 keys
    out = Buf(heads * d)
    good = dict(head_dim=D, n_head=heads, kv_bf16=0, q=g.qd, kbase=g.kd, vbase=g.vd, slots=g.slots_d, seq_len=g.base_d, max_seq=max_seq, d=d,
                scale=g.scale, Wp=Buf(data=wp(d)), out=out)
    assert probe(FUSED_PROJ, **good)[0] == -1                  # GVC_ERR_ARG
    ok128 = Buf(data=torch.tensor(mixed_base(n_slots, [slot], [127], other=3), dtype=torch.int32))
    for bad in (dict(head_dim=128), dict(d=1024), dict(n_head=1), dict(seq_len=None), dict(Wp=None)):
        assert probe(FUSED_PROJ, **{**good, "seq_len": ok128, **bad})[0] == -1, bad
    assert bool((out.bits() == PAT).all()) and out.guards_ok()
    assert probe(FUSED_PROJ, **dict(good, seq_len=ok128))[0] == 0


# ------------------------------------------------------------------ k_attn64_mfma ------------------------------------------------------------------
def a64_case(seed, regime, nw, mask_on, E, B, Tq, Tk, layout, fm16, excluded=None, what=None):
    """one k_attn64_mfma call.  layout "cv": ContentVec's [T][3E] rows q | k | v; "pc": the Perceiver's [Tk][depth * 3 * inner] rows, second
    of two layers, queries = the first Tq rows.  excluded [B][Tk] bool: the fmask.  -> (out Buf, idx, ref, tol, e32)"""
    heads, D, scale = E // 64, 64, 0.125
    keep = None if excluded is None else ~excluded
    limits = torch.full((B, Tq), Tk) if keep is None else keep.sum(dim=1).view(B, 1).expand(B, Tq).contiguous()
    q, kc, vc = make_inputs(seed, regime, D, heads, B, Tq, B, Tk, scale, limits)
    qh = q.permute(0, 2, 1, 3)
    full = torch.full((B, Tq), Tk)
    if keep is None:
        check_regime(regime, qh, kc, scale, full, what)
    ld, off = (3 * E, 0) if layout == "cv" else (6 * E, 3 * E)
    R = Tk + 2                                                                  # two rows past Tk, NaN like every column of another layer
    buf = torch.full((B, R, ld), NAN)
    buf[:, :Tq, off:off + E] = q.reshape(B, Tq, E)
    buf[:, :Tk, off + E:off + 2 * E] = kc.permute(0, 2, 1, 3).reshape(B, Tk, E)
    buf[:, :Tk, off + 2 * E:off + 3 * E] = vc.permute(0, 2, 1, 3).reshape(B, Tk, E)
    qkv = Buf(data=buf)
    ref = AO.attend(qh.double(), kc.double(), vc.double(), scale, full, keep, empty="nan")
    r32 = AO.attend(qh, kc, vc, scale, full, keep, empty="nan")
    live = torch.isfinite(ref)
    e32 = float((r32.double() - ref)[live].abs().max())
    tol = a64_tol(e32, ref[live])
    n, idx = out_idx(B * Tq, E, fm16)
    out = Buf(n)
    fm = None if excluded is None else Buf(data=excluded.to(torch.int32))
    ok(ATTN64, n_head=heads, batch=B, q=Buf.ptr(qkv, off), kbase=Buf.ptr(qkv, off + E), vbase=Buf.ptr(qkv, off + 2 * E), ld=ld, bs=R * ld, Tq=Tq, Tk=Tk,
       out=out, out_rows=Tq, E=E, scale=scale, out_fm16=fm16, nw=nw, mask=mask_on, fmask=fm)
    assert qkv.guards_ok()
    return out, idx, ref.permute(0, 2, 1, 3).reshape(B * Tq, E), tol, e32


def a64_check(family, out, idx, ref, tol, e32, what):
    err = check(out, idx, ref, tol, what)
    note(family, e32, err, tol)
    return err / tol


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("E", [128, 768])
def test_attn64_contentvec_layout(E, regime):
    """NW 4 as ContentVec launches it: MASK instantiation, nothing excluded"""
    worst = 0.0
    for T in (1, 15, 16, 17, 63, 64, 65, 130):
        for B, fm16 in ((1, 0), (3, 1), (3, 0), (1, 1)):
            what = ("attn64 cv", E, T, B, fm16, regime)
            r = a64_case(8000 + E + T, regime, 4, 1, E, B, T, T, "cv", fm16, torch.zeros(B, T, dtype=torch.bool), what)
            worst = max(worst, a64_check("k_attn64_mfma<true, 4>", *r, what))
            if fm16 == 0 and B == 3:          # MASK with nothing excluded = MASK off, bit for bit
                plain = a64_case(8000 + E + T, regime, 4, 0, E, B, T, T, "cv", fm16, None, what)
                a64_check("k_attn64_mfma<false, 4>", *plain, what)
                assert torch.equal(plain[0].bits(), r[0].bits()), ("an all-zero fmask changes the bits", what)
    print(f"[attn-modes] k_attn64_mfma<true, 4> E {E} {regime}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("regime", REGIMES)
def test_attn64_perceiver_layout(regime):
    """NW 16 as the Perceiver launches it: fewer key tiles than waves at the short end (idle waves carry m = -inf into the merge)"""
    E, worst = 128, 0.0
    for Tq, Tk in ((16, 17), (32, 48), (64, 255), (16, 256), (32, 257), (64, 300)):
        for B, fm16 in ((1, 0), (3, 1), (3, 0), (1, 1)):
            what = ("attn64 pc", Tq, Tk, B, fm16, regime)
            plain = a64_case(8500 + Tk, regime, 16, 0, E, B, Tq, Tk, "pc", fm16, None, what)
            worst = max(worst, a64_check("k_attn64_mfma<false, 16>", *plain, what))
            masked = a64_case(8500 + Tk, regime, 16, 1, E, B, Tq, Tk, "pc", fm16, torch.zeros(B, Tk, dtype=torch.bool), what)
            worst = max(worst, a64_check("k_attn64_mfma<true, 16>", *masked, what))
            assert torch.equal(plain[0].bits(), masked[0].bits()), ("an all-zero fmask changes the bits", what)
    print(f"[attn-modes] k_attn64_mfma<*, 16> {regime}: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("nw,layout,Tq,Tk", [(4, "cv", 130, 130), (4, "cv", 65, 65), (16, "pc", 32, 300), (16, "pc", 16, 48)])
def test_attn64_masks(nw, layout, Tq, Tk):
    B, E = 3, 128
    ntile = -(-Tk // 16)
    z = torch.zeros(B, Tk, dtype=torch.bool)
    tail, tile, wave, both = z.clone(), z.clone(), z.clone(), z.clone()
    for b in range(B):
        tail[b, Tk - 1 - 7 * b:] = True                       # padding tails: one key, and tails that cross a tile boundary
    tile[:, 16:32] = True                                      # a fully masked 16-key tile
    w = 1 if nw == 4 else 2
    for kt in range(w, ntile, nw):                             # every tile of one wave: it reaches the merge with m = -inf
        wave[:, kt * 16:(kt + 1) * 16] = True
    both[:] = wave
    both[1, Tk - 20:] = True
    both[2, :16] = True                                        # wave 0's first tile too
    fam = f"k_attn64_mfma<true, {nw}>"
    for regime in REGIMES:
        for name, ex in (("padding tail", tail), ("one tile", tile), ("one wave's tiles", wave), ("wave and tail", both)):
            for fm16 in (0, 1):
                what = ("attn64 mask", name, nw, Tq, Tk, regime, fm16)
                a64_check(fam, *a64_case(9000 + Tk, regime, nw, 1, E, B, Tq, Tk, layout, fm16, ex, what), what)
    # a batch element with every key excluded: the softmax of a row of -inf, NaN (tests/attn_oracle.py: empty="nan"); the others unharmed
    dead = tail.clone()
    dead[1] = True
    out, idx, ref, tol, e32 = a64_case(9000 + Tk, "uniform", nw, 1, E, B, Tq, Tk, layout, 0, dead, "dead batch element")
    got = out.bits().view(torch.float32)[idx].view(B, Tq, E).double()
    ref = ref.view(B, Tq, E)
    assert bool(torch.isnan(ref[1]).all()) and bool(torch.isnan(got[1]).all())
    assert float((got[[0, 2]] - ref[[0, 2]]).abs().max()) < tol and out.guards_ok()


def test_attn64_probe_refuses_bad_cases():
    z = Buf(data=torch.zeros(16 * 192))
    good = dict(n_head=1, batch=1, q=z, kbase=Buf.ptr(z, 64), vbase=Buf.ptr(z, 128), ld=192, bs=16 * 192, Tq=16, Tk=16, out=Buf(16 * 64), out_rows=16, E=64,
                scale=0.125, nw=4, mask=0)
    assert probe(ATTN64, **good)[0] == 0
    for bad in (dict(nw=8), dict(E=128), dict(ld=190), dict(Tk=0), dict(mask=1), dict(out_rows=8)):
        assert probe(ATTN64, **dict(good, **bad))[0] == -1, bad


# ------------------------------------------------------------------ report ------------------------------------------------------------------
def test_zz_report_measured_errors():
    """the per-family maxima (pytest -s).  Meaningful only for a full serial run of this file: STATS is filled by the tests above in file
    order, so a -k selection or a distributed run prints partial figures; the assertion repeats what every case asserted already"""
    for fam, (e32, err, ratio, n) in sorted(STATS.items()):
        print(f"[attn-modes] {fam}: {n} launches, max e32 {e32:.3e}, max kernel error {err:.3e}, worst error / bound {ratio:.3f}")
        assert ratio < 1.0
