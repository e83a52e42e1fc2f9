"""Every operand mode, epilogue and edge of the fp32 GEMM kernels (csrc/gemm.hip) alone, through the C-ABI test hook
gvc_gemm_probe_ex on buffers this file owns.

Rules of every case: inputs are seeded CPU tensors; the reference is fp64 arithmetic on the same fp32 values (tests/gemm_oracle.py,
itself checked against torch in tests/test_gemm_oracle_host.py); every output buffer is pre-filled with a NaN bit pattern and sits
between two guard regions of the same pattern; every element the operation owns must match the reference, and every element it does
not own (columns N..ldc-1, rows past M, gaps between batch planes, untouched cache positions, padding rows of fragment-major outputs,
the guards) must still hold the pattern bit for bit.  Padding rows of fragment-major A operands hold the NaN pattern too (the operand
conversion is its own probe call into a pattern-filled buffer), so a kernel that let them reach a stored element would fail.

Bounds: plain GEMM / conv / linear epilogues use tests/test_gpu_gemm.py's 2e-5 * sqrt(K / 256) * max(1, max|ref|) (K = the slice length
for raw split-K planes).  Cases through an approximated function (gelu, the merge's exp, LayerNorm's rsqrt) allow the larger of that
and 4x the error of a plain fp32 torch evaluation of the same formula against the fp64 oracle, measured on the case's own inputs on
the CPU -- never from the kernel's output.  Bit-equality is asserted only where the source promises it: split-K repeatability, the
completed rows of fused vs unfused LN + GEMM (the normalised rows turned out not to be, see the test), the bf16 cache vs the rounded
fp32 cache.  DESIGN.md "GEMM mode tests" records the matrix and the measured
figures."""
import ctypes as C
import itertools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as GO                      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAT = 0x7FC0BEEF            # a quiet NaN nobody computes
GUARD = 256                 # 4-byte elements on each side (keeps the 16-byte alignment of the payload)
TILED, SKINNY, SKINNY_LN, STRIP, STRIP_GEOM, LN_ROWS, LN_ROWS_B16, TO_FM16, TO_FM16_BF16 = range(9)
NAN = float("nan")


class Buf:
    """n 4-byte elements on the device between two guard regions; payload = `data` (fp32 / int32 CPU tensor) or the NaN pattern"""

    def __init__(self, n=None, data=None):
        if data is not None:
            data = data.contiguous().reshape(-1)
            n = data.numel()
        self.n = n
        self.raw = torch.full((n + 2 * GUARD,), PAT, dtype=torch.int32, device=DEV)
        self.t = self.raw[GUARD:GUARD + n]
        if data is not None:
            self.t.copy_(data.view(torch.int32))

    def ptr(self, off=0):
        return self.t.data_ptr() + 4 * off

    def bits(self):
        return self.t.cpu()

    def f32(self):
        return self.t.cpu().view(torch.float32)

    def guards_ok(self):
        raw = self.raw.cpu()
        return bool((raw[:GUARD] == PAT).all()) and bool((raw[GUARD + self.n:] == PAT).all())


def run(kind, **kw):
    """one probe call; Buf arguments become their payload address.  Returns (rc, sk_used)"""
    from genvc_amd import _lib
    c = _lib.GemmCase()
    c.kind = kind
    for k, v in kw.items():
        setattr(c, k, v.ptr() if isinstance(v, Buf) else v)
    rc = _lib.lib().gvc_gemm_probe_ex(C.byref(c), _lib.stream())
    return rc, c.sk_used


def ok(kind, **kw):
    rc, sk = run(kind, **kw)
    if rc != 0:
        from genvc_amd import _lib
        raise AssertionError(f"probe kind {kind} failed with {rc}: {_lib.lib().gvc_last_error().decode()}")
    return sk


def rm_idx(M, N, ld, off=0):
    return (torch.arange(M).view(M, 1) * ld + torch.arange(N).view(1, N) + off).reshape(-1)


def fm_idx(M, N):
    """flat FM16 positions of rows < M of an [ceil16(M)][N] matrix, row-major order of (m, n)"""
    return GO.fm16_perm(-(-M // 16) * 16, N)[:M].reshape(-1)


def check(buf, idx, ref, tol, what):
    """buf[idx] matches ref (fp64, same order) within tol; every other element and both guards still hold the pattern"""
    bits = buf.bits()
    owned = torch.zeros(buf.n, dtype=torch.bool)
    owned[idx] = True
    assert int(owned.sum()) == idx.numel(), what
    assert bool((bits[~owned] == PAT).all()), (what, "an element outside the result was written", int((bits[~owned] != PAT).sum()))
    assert buf.guards_ok(), (what, "guard region written")
    out = bits.view(torch.float32)[idx].double()
    assert bool(torch.isfinite(out).all()), (what, "non-finite result")
    err = float((out - ref.reshape(-1)).abs().max())
    assert err < tol, (what, err, tol)
    return err


def approx_tol(name, K, ref64, restated32):
    """bound of a case through an approximated function: max(project bound, 4 x the error of the fp32 torch restatement)"""
    e32 = float((restated32.double() - ref64).abs().max())
    base = GO.gemm_tol(K, ref64)
    tol = max(base, 4.0 * e32)
    print(f"[gemm-modes] {name}: fp32 restatement err {e32:.3e}, project bound {base:.3e}, bound used {tol:.3e}")
    return tol


def fm16_dev(x, bf16=False):
    """row-major CPU [M][K] -> device FM16 operand, converted by the layout kernel into a pattern-filled buffer: padding rows stay NaN"""
    M, K = x.shape
    Mp = -(-M // 16) * 16
    src = Buf(data=x)
    dst = Buf(Mp * K // (2 if bf16 else 1))
    ok(TO_FM16_BF16 if bf16 else TO_FM16, A=src, C=dst, M=M, K=K)
    return dst


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------ layout kernels ------------------------------------------------------------------
@pytest.mark.parametrize("N,K", [(16, 16), (48, 80), (128, 272)])
def test_layout_kernels_match_the_map(N, K):
    g = torch.Generator().manual_seed(N + K)
    x = GO.bf16_round(rnd(g, N, K))
    want = GO.to_fm16(x)
    got = fm16_dev(x)
    assert got.guards_ok() and torch.equal(got.bits(), want.view(torch.int32))
    got16 = fm16_dev(x, bf16=True)
    assert got16.guards_ok() and torch.equal(got16.bits().view(torch.int16), GO.bf16_bits(want).to(torch.int16))
    # fewer rows than the padded height: the padding rows are not written
    part = fm16_dev(x[:N - 5])
    bits, perm = part.bits(), GO.fm16_perm(N, K)
    assert torch.equal(bits[perm[:N - 5].reshape(-1)], x[:N - 5].reshape(-1).view(torch.int32))
    assert bool((bits[perm[N - 5:].reshape(-1)] == PAT).all())


# ------------------------------------------------------------------ tiled kernel ------------------------------------------------------------------
def test_tiled_edges_and_strides():
    g = torch.Generator().manual_seed(11)
    Ms, Ns, Ks = (1, 63, 64, 65, 130), (1, 20, 64, 80, 100), (4, 28, 36, 100, 132)
    A0, W0, b0 = rnd(g, 130, 132), rnd(g, 100, 132, scale=0.2), rnd(g, 100)
    worst = 0.0
    for M, N, K in itertools.product(Ms, Ns, Ks):
        lda, ldw, ldc = K + 4, K + 8, N + 3
        A = torch.full((M, lda), NAN)
        A[:, :K] = A0[:M, :K]
        W = torch.full((N, ldw), NAN)           # what lies between K and the leading dimension must never be read
        W[:, :K] = W0[:N, :K]
        ref = A0[:M, :K].double() @ W0[:N, :K].double().T + b0[:N].double()
        out = Buf((M + 2) * ldc)
        ok(TILED, A=Buf(data=A), W=Buf(data=W), C=out, bias=Buf(data=b0[:N]), M=M, N=N, K=K, lda=lda, ldw=ldw, ldc=ldc, batch=1)
        worst = max(worst, check(out, rm_idx(M, N, ldc), ref, GO.gemm_tol(K, ref), ("tiled edge", M, N, K)) / GO.gemm_tol(K, ref))
    print(f"[gemm-modes] tiled edges: worst err / bound {worst:.3f}")


def test_tiled_refuses_unaligned():
    z = Buf(data=torch.zeros(64 * 64))
    good = dict(A=z, W=z, C=Buf(64 * 64), M=8, N=8, K=8, lda=8, ldw=8, ldc=8, batch=1)
    assert run(TILED, **good)[0] == 0
    for bad in (dict(K=6), dict(lda=10), dict(ldw=9), dict(conv_cin=2, conv_tap_stride=8), dict(conv_cin=4, conv_tap_stride=6)):
        assert run(TILED, **dict(good, **bad))[0] != 0, bad


def _splitk_planes(work):
    """number of leading elements of the work buffer that were written"""
    return int((work.bits() != PAT).sum())


def test_tiled_splitk_rules_and_determinism():
    g = torch.Generator().manual_seed(12)
    # (M, N, K, batch, work_cap or None = exact, expected SK)
    cases = [(70, 40, 520, 1, 16 * 70 * 40, 4),          # first rule: 2 tiles -> K / 128 = 4 splits, the last one ends in a partial tile
             (8, 16, 2080, 1, 16 * 8 * 16, 16),          # 65 k tiles, 5 per split: splits 13..15 own none
             (8, 16, 2080, 1, 5 * 8 * 16, 5),            # work_cap forces the split down
             (8, 16, 2080, 1, 0, 1)]                     # no work buffer
    for M, N, K, batch, cap, SK in cases:
        A, W, b = rnd(g, M, K), rnd(g, N, K, scale=0.1), rnd(g, N)
        ref = A.double() @ W.double().T + b.double()
        outs = []
        for rep in range(2):
            out, work = Buf(M * N), Buf(max(cap, 1))
            ok(TILED, A=Buf(data=A), W=Buf(data=W), C=out, bias=Buf(data=b), M=M, N=N, K=K, lda=K, ldw=K, ldc=N, batch=batch,
               work=work if cap else None, work_cap=cap)
            check(out, rm_idx(M, N, N), ref, GO.gemm_tol(K, ref), ("split-K", M, N, K, cap))
            assert work.guards_ok()
            assert _splitk_planes(work) == (SK * M * N if SK > 1 else 0), ("planes written", _splitk_planes(work), SK)
            if SK == 16:         # the splits without a k tile contribute exact zeros
                assert bool((work.bits()[13 * M * N:] == 0).all())
            outs.append(out.bits())
        assert torch.equal(outs[0], outs[1]), "split-K is not repeatable"


def test_tiled_splitk_second_rule():
    """batch 16, M 500, N 48, K 2048: 128 tiles and a long K -> SK 4 (the ContentVec positional conv's rule)"""
    g = torch.Generator().manual_seed(13)
    B, M, N, K, SK = 16, 500, 48, 2048, 4
    step = 4 * K                                 # batch b's A starts 4 rows below batch b-1's: distinct operands, one small buffer
    A = rnd(g, M + 4 * (B - 1), K)
    W, b = rnd(g, B, N, K, scale=0.05), rnd(g, B, N)
    ref = torch.stack([A[4 * i:4 * i + M].double() @ W[i].double().T + b[i].double() for i in range(B)])
    gap = 32
    cbs = M * N + gap
    idx = torch.cat([rm_idx(M, N, N, i * cbs) for i in range(B)])
    outs = []
    for rep in range(2):
        out, work = Buf(B * cbs), Buf(B * SK * M * N)
        ok(TILED, A=Buf(data=A), W=Buf(data=W), C=out, bias=Buf(data=b), M=M, N=N, K=K, lda=K, ldw=K, ldc=N, batch=B, a_batch_stride=step,
           w_batch_stride=N * K, c_batch_stride=cbs, bias_batch_stride=N, work=work, work_cap=B * SK * M * N)
        check(out, idx, ref, GO.gemm_tol(K, ref), "split-K second rule")
        assert work.guards_ok() and _splitk_planes(work) == B * SK * M * N
        outs.append(out.bits())
    assert torch.equal(outs[0], outs[1])


def test_tiled_batches():
    g = torch.Generator().manual_seed(14)
    M, N, K = 70, 40, 36
    # three dense batches, planes separated by gaps
    A, W, b = rnd(g, 3, M, K), rnd(g, 3, N, K, scale=0.2), rnd(g, 3, N)
    ref = torch.einsum("bmk,bnk->bmn", A.double(), W.double()) + b.double().unsqueeze(1)
    cbs = M * N + 20
    out = Buf(3 * cbs)
    ok(TILED, A=Buf(data=A), W=Buf(data=W), C=out, bias=Buf(data=b), M=M, N=N, K=K, lda=K, ldw=K, ldc=N, batch=3, a_batch_stride=M * K,
       w_batch_stride=N * K, c_batch_stride=cbs, bias_batch_stride=N)
    check(out, torch.cat([rm_idx(M, N, N, i * cbs) for i in range(3)]), ref, GO.gemm_tol(K, ref), "dense batches")

    # grouped conv over one [T][E] buffer, batch = group: A / C / resid move by cg inside a row, bias by cg; and the two-level form
    # (outer = utterance with its own plane stride); weights and bias move by the inner index only
    for outer in (1, 3):
        G_, cg, kp, T = (3, 8, 5, 45) if outer == 1 else (2, 8, 5, 45)
        E, pad = G_ * cg, kp // 2
        x = rnd(g, outer, T + 2 * pad, E)
        x[:, :pad] = 0
        x[:, pad + T:] = 0
        w, bias = rnd(g, E, cg, kp, scale=0.2), rnd(g, E)
        conv = F.conv1d(x[:, pad:pad + T].double().transpose(1, 2), w.double(), bias.double(), padding=pad, groups=G_).transpose(1, 2)
        ref = x[:, pad:pad + T].double() + GO.gelu_erf(conv)
        conv32 = F.conv1d(x[:, pad:pad + T].transpose(1, 2), w, bias, padding=pad, groups=G_).transpose(1, 2)
        tol = approx_tol("tiled grouped conv + gelu_erf + resid", kp * cg, ref, x[:, pad:pad + T] + GO.gelu_erf(conv32))
        Wt = torch.stack([GO.conv_weight_matrix(w[i * cg:(i + 1) * cg]) for i in range(G_)])      # [G][cg][kp * cg]
        xb = Buf(data=x)
        xp_bs, o_bs = (T + 2 * pad) * E, T * E + 24
        out = Buf(outer * o_bs)
        kw = dict(A=xb, W=Buf(data=Wt), C=out, bias=Buf(data=bias), M=T, N=cg, K=kp * cg, lda=E, ldw=kp * cg, ldc=E, batch=outer * G_,
                  conv_cin=cg, conv_tap_stride=E, w_batch_stride=cg * kp * cg, bias_batch_stride=cg, act=GO.ACT_GELU_ERF,
                  resid=xb.ptr(pad * E), ldr=E)
        if outer == 1:
            kw.update(a_batch_stride=cg, c_batch_stride=cg, resid_batch_stride=cg)
        else:
            kw.update(batch_inner=G_, a_batch_stride=cg, a_batch_stride2=xp_bs, c_batch_stride=cg, c_batch_stride2=o_bs,
                      resid_batch_stride=cg, resid_batch_stride2=xp_bs)
        ok(TILED, **kw)
        check(out, torch.cat([rm_idx(T, E, E, i * o_bs) for i in range(outer)]), ref, tol, ("grouped conv batches", outer))


def test_tiled_implicit_conv():
    """dilated conv over a padded time-major buffer laid out as the vocoder lays it out, leaky-ReLU applied while A is staged"""
    g = torch.Generator().manual_seed(15)
    P, Co, B = 28, 24, 2
    worst = 0.0
    for Ci, taps, dil, T in itertools.product((4, 20, 32), (1, 3, 7, 11), (1, 3, 5), (37, 130)):
        if taps == 1 and dil > 1:
            continue
        pad = dil * (taps - 1) // 2
        x = rnd(g, B, T, Ci)
        x[torch.rand(B, T, Ci, generator=g) < 0.1] = 0.0          # exact zeros next to negative values
        w, bias = rnd(g, Co, Ci, taps, scale=0.2), rnd(g, Co)
        xp = torch.zeros(B, T + 2 * P, Ci)
        xp[:, P:P + T] = x
        K = taps * Ci
        bs_in, bs_out = (T + 2 * P) * Ci, (T + 2 * P) * Co
        xb, wb, bb = Buf(data=xp), Buf(data=GO.conv_weight_matrix(w)), Buf(data=bias)
        idx = torch.cat([rm_idx(T, Co, Co, i * bs_out + P * Co) for i in range(B)])
        for slope in (0.0, 0.1):
            xin = x.double() if slope == 0.0 else F.leaky_relu(x.double(), slope)
            ref = F.conv1d(xin.transpose(1, 2), w.double(), bias.double(), padding=pad, dilation=dil).transpose(1, 2)
            out, work = Buf(B * bs_out), Buf(16 * B * T * Co)
            ok(TILED, A=xb.ptr((P - pad) * Ci), W=wb, C=out.ptr(P * Co), bias=bb, M=T, N=Co, K=K, lda=Ci, ldw=K, ldc=Co, batch=B,
               a_batch_stride=bs_in, c_batch_stride=bs_out, conv_cin=Ci, conv_tap_stride=dil * Ci, a_act=1 if slope else 0, a_slope=slope,
               work=work if T == 130 else None, work_cap=16 * B * T * Co)
            tol = GO.gemm_tol(K, ref)
            worst = max(worst, check(out, idx, ref, tol, ("implicit conv", Ci, taps, dil, T, slope)) / tol)
            assert work.guards_ok()
    print(f"[gemm-modes] implicit conv: worst err / bound {worst:.3f}")


EPILOGUES = ["gelu_new", "relu", "gelu_erf", "resid", "resid_inplace", "resid2", "out_scale", "hifigan"]


def _epi_case(g, M, N, name):
    """(probe fields as CPU tensors, fp64 / fp32 epilogue functions) of one named epilogue"""
    b, r1, r2 = rnd(g, N), rnd(g, M, N), rnd(g, M, N)
    act = {"gelu_new": GO.ACT_GELU_NEW, "relu": GO.ACT_RELU, "gelu_erf": GO.ACT_GELU_ERF}.get(name, GO.ACT_NONE)
    resid = r1 if name in ("resid", "resid_inplace", "resid2", "hifigan") else None
    resid2 = r2 if name in ("resid2", "hifigan") else None
    scale = {"out_scale": 0.37, "hifigan": 1.0 / 3.0}.get(name, 0.0)

    def fn(acc):
        t = acc.dtype
        return GO.epilogue(acc, b.to(t), act, None if resid is None else resid.to(t), None if resid2 is None else resid2.to(t), scale)
    return b, act, resid, resid2, scale, fn


@pytest.mark.parametrize("name", EPILOGUES)
def test_tiled_epilogues(name):
    """each epilogue once in the kernel (SK = 1: no work buffer) and once through k_splitk_epilogue (SK = 4)"""
    g = torch.Generator().manual_seed(16)
    M, N, K, ld = 70, 40, 520, 44
    A, W = rnd(g, M, K), rnd(g, N, K, scale=0.1)
    b, act, resid, resid2, scale, fn = _epi_case(g, M, N, name)
    ref = fn(A.double() @ W.double().T)
    tol = approx_tol("tiled epilogue " + name, K, ref, fn(A @ W.T))
    idx = rm_idx(M, N, ld)
    results = []
    for split in (False, True):
        out, work = Buf(M * ld), Buf(4 * M * N)
        kw = dict(A=Buf(data=A), W=Buf(data=W), C=out, bias=Buf(data=b), act=act, out_scale=scale, M=M, N=N, K=K, lda=K, ldw=K, ldc=ld, batch=1,
                  ldr=ld, work=work if split else None, work_cap=4 * M * N)
        if resid is not None:
            padded = torch.full((M, ld), NAN)
            padded[:, :N] = resid
            if name == "resid_inplace":             # the residual lives in C itself; the columns past N keep the pattern
                out.t[idx.to(DEV)] = resid.reshape(-1).view(torch.int32).to(DEV)
                kw["resid"] = out
            else:
                kw["resid"] = Buf(data=padded)
        if resid2 is not None:
            padded2 = torch.full((M, ld), NAN)
            padded2[:, :N] = resid2
            kw["resid2"] = Buf(data=padded2)
        ok(TILED, **kw)
        check(out, idx, ref, tol, ("tiled epilogue", name, split))
        assert _splitk_planes(work) == (4 * M * N if split else 0)
        results.append(out.f32()[idx])
    assert float((results[0] - results[1]).abs().max()) < tol


# ------------------------------------------------------------------ skinny kernel ------------------------------------------------------------------
SKINNY_M = (1, 15, 16, 17, 32, 33, 49, 64, 65, 81, 97, 113, 128)        # MT 1..8: the MT <= 2, MT = 3 and MT >= 4 paths


def _skinny_shapes():
    for M in SKINNY_M:
        for K in (256, 192):
            yield M, K
    for M, K in ((1, 64), (40, 64), (70, 64), (128, 64), (9, 512), (70, 512)):       # kw = 16 with 4 waves; K = 512 allows SK = 8
        yield M, K


def test_skinny_shapes_and_raw_planes():
    g = torch.Generator().manual_seed(21)
    worst = 0.0
    A0, W0, b0 = rnd(g, 128, 512), rnd(g, 48, 512, scale=0.1), rnd(g, 48)
    for (M, K), N in itertools.product(_skinny_shapes(), (16, 48)):
        A, W, b = A0[:M, :K].contiguous(), W0[:N, :K].contiguous(), b0[:N].contiguous()
        Af, Wf, bb = fm16_dev(A), fm16_dev(W), Buf(data=b)
        ldc = N + 4
        for SK in (s for s in (1, 2, 4, 8) if K % (64 * s) == 0):
            out, work = Buf(M * ldc), Buf(SK * M * N)
            ok(SKINNY, A=Af, W=Wf, C=out, bias=bb, M=M, N=N, K=K, lda=K, ldw=K, ldc=ldc, sk=SK, work=work, work_cap=SK * M * N)
            what = ("skinny", M, N, K, SK)
            if SK == 1:
                ref = A.double() @ W.double().T + b.double()
                worst = max(worst, check(out, rm_idx(M, N, ldc), ref, GO.gemm_tol(K, ref), what) / GO.gemm_tol(K, ref))
                assert _splitk_planes(work) == 0 and work.guards_ok()
            else:            # raw planes: no bias, no C
                ks = K // SK
                ref = torch.stack([A[:, s * ks:(s + 1) * ks].double() @ W[:, s * ks:(s + 1) * ks].double().T for s in range(SK)])
                check(work, torch.arange(SK * M * N), ref, GO.gemm_tol(ks, ref), what)
                full = A.double() @ W.double().T
                err = float((work.f32().view(SK, M, N).double().sum(0) - full).abs().max())
                assert err < GO.gemm_tol(K, full), (what, "planes do not sum to the product", err)
                assert _splitk_planes(out) == 0 and out.guards_ok()
    print(f"[gemm-modes] skinny shapes: worst err / bound {worst:.3f}")


@pytest.mark.parametrize("K", [256, 192])
@pytest.mark.parametrize("M", [9, 40, 70])             # MT 1, 3, 5
def test_skinny_epilogues(M, K):
    g = torch.Generator().manual_seed(22 + M + K)
    N = 32
    Mp = -(-M // 16) * 16
    A, W = rnd(g, M, K), rnd(g, N, K, scale=0.1)
    Af, Wf = fm16_dev(A), fm16_dev(W)
    acc64, acc32 = A.double() @ W.double().T, A @ W.T
    base = dict(A=Af, W=Wf, M=M, N=N, K=K, lda=K, ldw=K, ldc=N, sk=1)
    b, r = rnd(g, N), rnd(g, M, N)
    bb = Buf(data=b)
    # fragment-major C, alone and with a fragment-major residual
    for with_resid in (False, True):
        ref = GO.epilogue(acc64, b.double(), GO.ACT_NONE, r.double() if with_resid else None)
        out = Buf(Mp * N)
        kw = dict(base, C=out, bias=bb, c_fm16=1)
        if with_resid:
            kw.update(resid=Buf(data=GO.to_fm16(r, fill=NAN)), resid_fm16=1, ldr=N)
        ok(SKINNY, **kw)
        check(out, fm_idx(M, N), ref, GO.gemm_tol(K, ref), ("skinny c_fm16", M, K, with_resid))
    # GEGLU: (x_j, gate_j) column pairs -> column j of a fragment-major [M][N / 2]
    ref = GO.geglu(acc64, b.double())
    out = Buf(Mp * (N // 2))
    ok(SKINNY, **dict(base, C=out, bias=bb, geglu=1))
    check(out, fm_idx(M, N // 2), ref, approx_tol("skinny geglu", K, ref, GO.geglu(acc32, b)), ("skinny geglu", M, K))
    # activations
    for act, nm in ((GO.ACT_GELU_NEW, "gelu_new"), (GO.ACT_RELU, "relu"), (GO.ACT_GELU_ERF, "gelu_erf")):
        ref = GO.epilogue(acc64, b.double(), act)
        out = Buf(M * N)
        ok(SKINNY, **dict(base, C=out, bias=bb, act=act))
        check(out, rm_idx(M, N, N), ref, approx_tol("skinny " + nm, K, ref, GO.epilogue(acc32, b, act)), ("skinny act", nm, M, K))
    # a plain residual, second residual and scale: the prefetched epilogues and the tiled kernel's agree on the same case
    r2 = rnd(g, M, N)
    ref = GO.epilogue(acc64, b.double(), GO.ACT_NONE, r.double(), r2.double(), 0.5)
    tol = GO.gemm_tol(K, ref)
    out_s, out_t = Buf(M * N), Buf(M * N)
    epi = dict(bias=bb, resid=Buf(data=r), resid2=Buf(data=r2), ldr=N, out_scale=0.5)
    ok(SKINNY, **dict(base, C=out_s, **epi))
    ok(TILED, **dict(base, A=Buf(data=A), W=Buf(data=W), C=out_t, batch=1, **epi))
    check(out_s, rm_idx(M, N, N), ref, tol, ("skinny resid", M, K))
    check(out_t, rm_idx(M, N, N), ref, tol, ("tiled resid", M, K))
    assert float((out_s.f32() - out_t.f32()).abs().max()) < tol


def _qkv_case(g, n_entries, T, d, n_head, K):
    hd = d // n_head
    M, N = n_entries * T, 3 * d
    n_slots = n_entries + 3
    slots = torch.randperm(n_slots, generator=g)[:n_entries].to(torch.int32)
    base = torch.randint(1, 6, (n_slots,), generator=g).to(torch.int32)
    max_seq = 5 + T + 3
    A, W, b = rnd(g, M, K), rnd(g, N, K, scale=0.1), rnd(g, N)
    kc = torch.full((n_slots, n_head, max_seq, hd), NAN, dtype=torch.float64)
    vc = kc.clone()
    q = GO.qkv_scatter(A.double() @ W.double().T, b.double(), GO.ACT_NONE, d, n_head, hd, T, slots, base, kc, vc)
    return dict(M=M, N=N, K=K, d=d, n_head=n_head, head_dim=hd, T=T, max_seq=max_seq, A=A, W=W, b=b, slots=slots, base=base, q=q, kc=kc, vc=vc)


def _run_qkv(kind, c, extra):
    """the scatter with an fp32 and a bf16 cache; q and the fp32 cache against fp64, the bf16 cache bit-equal to the rounded fp32 one"""
    Af, Wf = fm16_dev(c["A"]), fm16_dev(c["W"])
    n_cache = c["kc"].numel()
    tol = GO.gemm_tol(c["K"], torch.cat([c["q"].reshape(-1), c["kc"][~c["kc"].isnan()], c["vc"][~c["vc"].isnan()]]))
    owned = (~c["kc"].isnan()).reshape(-1).nonzero().reshape(-1)
    assert torch.equal(owned, (~c["vc"].isnan()).reshape(-1).nonzero().reshape(-1))
    caches = {}
    for bf16 in (0, 1):
        q, kc, vc = Buf(c["M"] * c["d"]), Buf(n_cache // (2 if bf16 else 1)), Buf(n_cache // (2 if bf16 else 1))
        ok(kind, A=Af, W=Wf, C=q, bias=Buf(data=c["b"]), M=c["M"], N=c["N"], K=c["K"], lda=c["K"], ldw=c["K"], ldc=c["d"], qkv=1, d=c["d"],
           n_head=c["n_head"], head_dim=c["head_dim"], max_seq=c["max_seq"], T=c["T"], kcache=kc, vcache=vc, kv_bf16=bf16,
           slots=Buf(data=c["slots"]), base_len=Buf(data=c["base"]), **extra)
        check(q, rm_idx(c["M"], c["d"], c["d"]), c["q"], tol, ("qkv q", kind, bf16))
        if not bf16:
            check(kc, owned, c["kc"].reshape(-1)[owned], tol, ("qkv k cache", kind))
            check(vc, owned, c["vc"].reshape(-1)[owned], tol, ("qkv v cache", kind))
            caches[0] = (kc.f32(), vc.f32())
        else:
            assert kc.guards_ok() and vc.guards_ok()
            pat16 = torch.tensor([PAT & 0xFFFF, PAT >> 16], dtype=torch.int32).repeat(n_cache // 2).to(torch.int16)
            for got, f32 in ((kc, caches[0][0]), (vc, caches[0][1])):
                want = pat16.clone()
                want[owned] = GO.bf16_bits(f32[owned]).to(torch.int16)
                assert torch.equal(got.bits().view(torch.int16), want), ("bf16 cache differs from the rounded fp32 cache", kind)


@pytest.mark.parametrize("n_head", [2, 1])
@pytest.mark.parametrize("n_entries", [1, 3, 8])
def test_skinny_qkv_scatter_8_waves(n_entries, n_head):
    g = torch.Generator().manual_seed(23 + n_entries)
    _run_qkv(SKINNY, _qkv_case(g, n_entries, 16, 64, n_head, 256), dict(sk=1))


@pytest.mark.parametrize("n_entries", [4, 6, 8])
def test_skinny_qkv_scatter_4_waves_two_items_per_thread(n_entries):
    """K = 192 runs 4 waves; with MT >= 5 a thread stores a second row 64 below its first, which belongs to another batch entry: its
    slot and cached length must be that entry's (they used to be the first row's)"""
    g = torch.Generator().manual_seed(24 + n_entries)
    _run_qkv(SKINNY, _qkv_case(g, n_entries, 16, 192, 3, 192), dict(sk=1))


@pytest.mark.parametrize("K", [256, 192])
def test_skinny_bf16_weights(K):
    g = torch.Generator().manual_seed(25)
    N = 48
    for M in (9, 40, 70):
        A, W, b = rnd(g, M, K), GO.bf16_round(rnd(g, N, K, scale=0.1)), rnd(g, N)
        ref = A.double() @ W.double().T + b.double()
        out = Buf(M * N)
        ok(SKINNY, A=fm16_dev(A), W=fm16_dev(W, bf16=True), w_bf16=1, C=out, bias=Buf(data=b), M=M, N=N, K=K, lda=K, ldw=K, ldc=N, sk=1)
        check(out, rm_idx(M, N, N), ref, GO.gemm_tol(K, ref), ("skinny bf16 weights", M, K))


@pytest.mark.parametrize("nc", [2, 4])
@pytest.mark.parametrize("M", [9, 25])
def test_skinny_attention_partials(M, nc):
    """A merged from per-chunk softmax partials (o, m, l) with widely different maxima; only states the attention kernel produces"""
    g = torch.Generator().manual_seed(26 + M + nc)
    heads, hd, N = 4, 64, 48
    K = heads * hd
    part = torch.zeros(M, heads, nc, hd + 4)
    part[..., hd] = rnd(g, M, heads, nc, scale=12.0)                       # m: finite, far apart
    part[..., hd + 1] = torch.rand(M, heads, nc, generator=g) * 30 + 1.0     # l >= 1 (the chunk's maximum contributes e^0)
    part[..., :hd] = rnd(g, M, heads, nc, hd) * part[..., hd + 1:hd + 2]     # o = sum p v, |o| <~ l |v|
    part[..., hd + 2:] = NAN                                                 # the tuple's padding is never read
    W, b = rnd(g, N, K, scale=0.1), rnd(g, N)
    ref = GO.att_merge(part[..., :hd + 2].double(), hd) @ W.double().T + b.double()
    r32 = GO.att_merge(part[..., :hd + 2], hd) @ W.T + b
    out = Buf(M * N)
    ok(SKINNY, att_part=Buf(data=part), att_nc=nc, att_heads=heads, att_hd=hd, W=fm16_dev(W), C=out, bias=Buf(data=b), M=M, N=N, K=K, lda=K,
       ldw=K, ldc=N, sk=1)
    check(out, rm_idx(M, N, N), ref, approx_tol("skinny attention partials", K, ref, r32), ("attention partials", M, nc))


# ------------------------------------------------------------------ skinny + LN, row kernels ------------------------------------------------------------------
@pytest.mark.parametrize("K", [256, 512, 768, 1024])
def test_skinny_ln_fused_vs_fp64_and_unfused(K):
    g = torch.Generator().manual_seed(31 + K)
    N = 48
    for rows, with_part, bf16 in itertools.product((1, 8, 9, 16), (False, True), (False, True)):
        x = rnd(g, rows, K, scale=2.0) + 0.5
        part, pb = (rnd(g, 4, rows, K), rnd(g, K)) if with_part else (None, None)
        lw, lb = rnd(g, K) + 1.0, rnd(g, K, scale=0.2)
        W, b = rnd(g, N, K, scale=0.1), rnd(g, N)
        if bf16:
            W = GO.bf16_round(W)
        v64 = GO.row_complete(x.double(), None if pb is None else pb.double(), None if part is None else part.double())
        ref = GO.layer_norm(v64, lw.double(), lb.double()) @ W.double().T + b.double()
        v32 = GO.row_complete(x, pb, part)
        tol = approx_tol("skinny+LN", K, ref, GO.layer_norm(v32, lw, lb) @ W.T + b)
        what = ("skinny+LN", rows, K, with_part, bf16)
        Wf, bb, xb = fm16_dev(W, bf16=bf16), Buf(data=b), Buf(data=x)
        lnw, lnb = Buf(data=lw), Buf(data=lb)
        pk = dict(part=Buf(data=part), pbias=Buf(data=pb), ln_sk=4) if with_part else {}
        out, xo = Buf(rows * N), Buf(rows * K)
        ok(SKINNY_LN, W=Wf, w_bf16=int(bf16), C=out, bias=bb, M=rows, N=N, K=K, ldw=K, ldc=N, x_in=xb, x_out=xo, ln_w=lnw, ln_b=lnb,
           ln_rows=rows, **pk)
        check(out, rm_idx(rows, N, N), ref, tol, what)
        check(xo, torch.arange(rows * K), v64, 1e-6 * 6 * float(v64.abs().max()), what + ("x_out",))       # five fp32 additions, half an ulp each
        # the row kernel followed by the skinny GEMM on the same data.  The source used to call the fused result bit-identical to this;
        # it is not (the LayerNorm is compiled into each kernel on its own and a row's mean / rstd can differ in the last bit: measured
        # through identity weights, whole rows differ by up to 1.5e-6 on O(1) values), so both are held to the fp64 bound and only the completed rows,
        # which are additions in one fixed order, must agree in bits
        a_fm, xo2, out2 = Buf(16 * K), Buf(rows * K), Buf(rows * N)
        ok(LN_ROWS, x_in=xb, x_out=xo2, C=a_fm, c_fm16=1, M=rows, K=K, ln_w=lnw, ln_b=lnb, **pk)
        ok(SKINNY, A=a_fm, W=Wf, w_bf16=int(bf16), C=out2, bias=bb, M=rows, N=N, K=K, lda=K, ldw=K, ldc=N, sk=1)
        check(out2, rm_idx(rows, N, N), ref, tol, what + ("unfused",))
        assert torch.equal(xo.bits(), xo2.bits()), what + ("x_out differs in bits",)


@pytest.mark.parametrize("d", [256, 768, 2048])
def test_ln_sum_rows(d):
    g = torch.Generator().manual_seed(32 + d)
    rows = 5
    for SK in (0, 1, 3, 8):
        x = rnd(g, rows, d, scale=2.0) + 0.5
        part, pb = (rnd(g, SK, rows, d), rnd(g, d)) if SK else (None, None)
        lw, lb = rnd(g, d) + 1.0, rnd(g, d, scale=0.2)
        v64 = GO.row_complete(x.double(), None if pb is None else pb.double(), None if part is None else part.double())
        a64 = GO.layer_norm(v64, lw.double(), lb.double())
        tol_a = approx_tol("ln_sum_rows", 256, a64, GO.layer_norm(GO.row_complete(x, pb, part), lw, lb))
        tol_x = 1e-6 * (SK + 2) * float(v64.abs().max())                 # SK + 1 fp32 additions, half an ulp each
        pk = dict(part=Buf(data=part), pbias=Buf(data=pb), ln_sk=SK) if SK else {}
        for mode in ("no_ln", "row_major", "fm16_inplace"):
            xb = Buf(data=x)
            xo = xb if mode == "fm16_inplace" else Buf(rows * d)
            a = Buf(16 * d if mode == "fm16_inplace" else rows * d)
            kw = dict(x_in=xb, x_out=xo, C=a, M=rows, K=d, **pk)
            if mode != "no_ln":
                kw.update(ln_w=Buf(data=lw), ln_b=Buf(data=lb), c_fm16=int(mode == "fm16_inplace"))
            ok(LN_ROWS, **kw)
            what = ("ln_sum_rows", d, SK, mode)
            check(xo, torch.arange(rows * d), v64, tol_x, what + ("x_out",))
            if mode == "no_ln":
                assert _splitk_planes(a) == 0 and a.guards_ok()
            else:
                check(a, fm_idx(rows, d) if mode == "fm16_inplace" else torch.arange(rows * d), a64, tol_a, what)


def _fb16_perm(M, K):
    """bf16 fragment-major layout of the matrix-core GEMMs (include/genvc_hip.h, gvc_fb16_index): (16 rows x 32 k) blocks of 64
    fragments of 8 consecutive k, fragment (m % 16) + 16 * ((k % 32) / 8)"""
    m, k = torch.arange(M).view(M, 1), torch.arange(K).view(1, K)
    return (m // 16 * (K // 32) + k // 32) * 512 + (m % 16 + 16 * (k % 32 // 8)) * 8 + k % 8


@pytest.mark.parametrize("d", [256, 768])
def test_ln_sum_rows_b16(d):
    g = torch.Generator().manual_seed(33 + d)
    rows = 5
    for SK in (0, 4):
        x = rnd(g, rows, d, scale=2.0) + 0.5
        part, pb = (rnd(g, SK, rows, d), rnd(g, d)) if SK else (None, None)
        v64 = GO.row_complete(x.double(), None if pb is None else pb.double(), None if part is None else part.double())
        pk = dict(part=Buf(data=part), pbias=Buf(data=pb), ln_sk=SK) if SK else {}
        xo, a16, stats = Buf(rows * d), Buf(16 * d // 2), Buf(2 * rows)
        ok(LN_ROWS_B16, x_in=Buf(data=x), x_out=xo, C=a16, stats=stats, M=rows, K=d, **pk)
        what = ("ln_sum_rows_b16", d, SK)
        check(xo, torch.arange(rows * d), v64, 1e-6 * (SK + 2) * float(v64.abs().max()), what + ("x_out",))
        # the rounded row = RNE of the completed fp32 row (the device's, checked above), in the fragment-major bf16 layout
        completed = xo.f32().view(rows, d)
        want = torch.tensor([PAT & 0xFFFF, PAT >> 16], dtype=torch.int32).repeat(16 * d // 2).to(torch.int16)
        want[_fb16_perm(16, d)[:rows].reshape(-1)] = GO.bf16_bits(completed).reshape(-1).to(torch.int16)
        assert a16.guards_ok() and torch.equal(a16.bits().view(torch.int16), want), what
        # (mean, rstd) of the ROUNDED row
        rounded = GO.bf16_round(completed)
        mean, rstd = GO.row_stats(rounded.double())
        ref = torch.stack([mean, rstd], dim=1)
        m32, r32 = GO.row_stats(rounded)
        check(stats, torch.arange(2 * rows), ref, approx_tol("ln_sum_rows_b16 stats", 256, ref, torch.stack([m32, r32], dim=1)), what + ("stats",))


# ------------------------------------------------------------------ strip kernel ------------------------------------------------------------------
def _check_planes(work, SK, M, N, A, W, kb, what):
    """raw planes of a K split over 16-wide k blocks: plane s covers blocks [s * kb / SK, (s + 1) * kb / SK)"""
    refs = []
    for s in range(SK):
        lo, hi = 16 * (s * kb // SK), 16 * ((s + 1) * kb // SK)
        refs.append(A[:, lo:hi].double() @ W[:, lo:hi].double().T)
    ref = torch.stack(refs)
    check(work, torch.arange(SK * M * N), ref, GO.gemm_tol(16 * -(-kb // SK), ref), what)
    full = A.double() @ W.double().T
    assert float((work.f32()[:SK * M * N].view(SK, M, N).double().sum(0) - full).abs().max()) < GO.gemm_tol(16 * kb, full), what


@pytest.mark.parametrize("w", range(1, 10))
def test_strip_forced_geometry(w):
    """every width (M tiles per workgroup) at shapes small enough to run in no time: fewer k blocks than one stage, a stage tail for
    the 8-block stages (w <= 4) and the 4-block stages (w >= 5), one and three n blocks, with and without a K split"""
    g = torch.Generator().manual_seed(40 + w)
    cases = [(16 * w - 3, w)] + ([(150, 4)] if w == 4 else [])           # M = 150, width 4: groups of 3, 3 and 4 tiles
    for (M, mtw), K, N in itertools.product(cases, (64, 80, 144, 272), (64, 192)):
        A, W, b = rnd(g, M, K), rnd(g, N, K, scale=0.1), rnd(g, N)
        Af, Wf, bb = fm16_dev(A), fm16_dev(W), Buf(data=b)
        ref = A.double() @ W.double().T + b.double()
        ldc = N + 4
        for SK in (1, 2):
            out, work = Buf((M + 1) * ldc), Buf(SK * M * N)
            kw = dict(A=Af, W=Wf, C=out, bias=bb, M=M, N=N, K=K, lda=K, ldw=K, ldc=ldc, mtw=mtw, sk=SK, work=work, work_cap=SK * M * N)
            if (K // 16) // SK < 4:
                assert run(STRIP_GEOM, **kw)[0] != 0, ("a split the kernel cannot run was accepted", M, K, SK)
                continue
            ok(STRIP_GEOM, **kw)
            check(out, rm_idx(M, N, ldc), ref, GO.gemm_tol(K, ref), ("strip geometry", mtw, M, N, K, SK))
            assert work.guards_ok() and _splitk_planes(work) == (SK * M * N if SK > 1 else 0)


@pytest.mark.parametrize("M", [17, 129, 300])
def test_strip_chooser_and_raw_partials(M):
    g = torch.Generator().manual_seed(50 + M)
    N, K = 64, 512
    kb = K // 16
    A, W, b = rnd(g, M, K), rnd(g, N, K, scale=0.1), rnd(g, N)
    Af, Wf, bb = fm16_dev(A), fm16_dev(W), Buf(data=b)
    ref = A.double() @ W.double().T + b.double()
    for sk_max, raw in itertools.product((1, 8), (0, 1)):
        out, work = Buf(M * N), Buf(8 * M * N)
        sk = ok(STRIP, A=Af, W=Wf, C=out, bias=bb, M=M, N=N, K=K, lda=K, ldw=K, ldc=N, sk=sk_max, raw_partials=raw, work=work, work_cap=8 * M * N)
        what = ("strip chooser", M, sk_max, raw, sk)
        print(f"[gemm-modes] strip chooser M={M} sk_max={sk_max} raw={raw}: sk_used {sk}")
        assert 1 <= sk <= sk_max
        if raw:              # the planes stay in `work` (one plane even without a split) and C is not touched
            assert _splitk_planes(out) == 0 and out.guards_ok()
            full = Buf(sk * M * N, data=work.f32()[:sk * M * N])
            assert _splitk_planes(work) == sk * M * N and work.guards_ok()
            _check_planes(full, sk, M, N, A, W, kb, what)
        else:
            check(out, rm_idx(M, N, N), ref, GO.gemm_tol(K, ref), what)
            assert _splitk_planes(work) == (sk * M * N if sk > 1 else 0)


def test_strip_epilogues():
    g = torch.Generator().manual_seed(60)
    M, N, K = 45, 64, 144
    Mp = 48
    A, W, b, r = rnd(g, M, K), rnd(g, N, K, scale=0.1), rnd(g, N), rnd(g, M, N)
    Af, Wf, bb = fm16_dev(A), fm16_dev(W), Buf(data=b)
    acc64, acc32 = A.double() @ W.double().T, A @ W.T
    for geom in ((STRIP, dict(sk=1)), (STRIP_GEOM, dict(mtw=2, sk=1)), (STRIP_GEOM, dict(mtw=3, sk=2))):
        kind, base = geom[0], dict(geom[1], A=Af, W=Wf, M=M, N=N, K=K, lda=K, ldw=K, ldc=N, bias=bb)
        if base["sk"] > 1:
            base.update(work=Buf(2 * M * N), work_cap=2 * M * N)
        ref = acc64 + b.double()
        out = Buf(Mp * N)
        ok(kind, **dict(base, C=out, c_fm16=1))
        check(out, fm_idx(M, N), ref, GO.gemm_tol(K, ref), ("strip c_fm16", geom))
        ref = GO.epilogue(acc64, b.double(), GO.ACT_NONE, r.double())
        out = Buf(data=r)                       # in-place residual
        ok(kind, **dict(base, C=out, resid=out, ldr=N))
        check(out, rm_idx(M, N, N), ref, GO.gemm_tol(K, ref), ("strip in-place resid", geom))
        ref = GO.epilogue(acc64, b.double(), GO.ACT_GELU_NEW)
        out = Buf(M * N)
        ok(kind, **dict(base, C=out, act=GO.ACT_GELU_NEW))
        check(out, rm_idx(M, N, N), ref, approx_tol("strip gelu_new", K, ref, GO.epilogue(acc32, b, GO.ACT_GELU_NEW)), ("strip gelu_new", geom))
        Wr = GO.bf16_round(W)
        ref = A.double() @ Wr.double().T + b.double()
        out = Buf(M * N)
        ok(kind, **dict(base, W=fm16_dev(Wr, bf16=True), w_bf16=1, C=out))
        check(out, rm_idx(M, N, N), ref, GO.gemm_tol(K, ref), ("strip bf16 weights", geom))
    c = _qkv_case(g, 3, 16, 64, 2, 144)
    _run_qkv(STRIP, c, dict(sk=1))
    _run_qkv(STRIP_GEOM, c, dict(mtw=2, sk=1))


def test_strip_refusals():
    z = Buf(data=torch.zeros(64 * 64))
    good = dict(A=z, W=z, C=Buf(64 * 64), M=20, N=64, K=64, lda=64, ldw=64, ldc=64, sk=1, mtw=2)
    for kind in (STRIP, STRIP_GEOM):
        assert run(kind, **good)[0] == 0
        assert run(kind, **dict(good, N=48))[0] != 0                      # N % 64 != 0
        assert run(kind, **dict(good, raw_partials=1))[0] != 0            # raw partials without a work buffer
        assert run(kind, **dict(good, geglu=1))[0] != 0                   # epilogues gemm_store4 does not have
        assert run(kind, **dict(good, resid=z, ldr=64, resid_fm16=1))[0] != 0
    assert run(STRIP_GEOM, **dict(good, mtw=0))[0] != 0
    assert run(STRIP_GEOM, **dict(good, mtw=10))[0] != 0
    assert run(STRIP_GEOM, **dict(good, sk=2, work=Buf(2 * 20 * 64), work_cap=2 * 20 * 64))[0] != 0      # kb / SK = 2 < 4
    assert run(STRIP_GEOM, **dict(good, K=128, sk=2, A=Buf(data=torch.zeros(32 * 128)), W=Buf(data=torch.zeros(64 * 128)), lda=128, ldw=128,
                                  work=Buf(20 * 64), work_cap=20 * 64))[0] != 0                          # work too small for two planes
