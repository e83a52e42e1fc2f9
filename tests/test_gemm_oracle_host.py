"""tests/gemm_oracle.py against torch's own functions (CPU): the restatements the GPU GEMM mode tests trust are checked here against
independent implementations, not against themselves."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_oracle as GO                      # noqa: E402


@pytest.mark.parametrize("M,K", [(16, 16), (48, 80), (128, 272)])
def test_fm16_is_a_bijection_of_contiguous_blocks(M, K):
    p = GO.fm16_perm(M, K)
    assert sorted(p.reshape(-1).tolist()) == list(range(M * K))
    for mb in range(M // 16):
        for kb in range(K // 16):
            blk = p[mb * 16:(mb + 1) * 16, kb * 16:(kb + 1) * 16].reshape(-1)
            assert int(blk.min()) == (mb * (K // 16) + kb) * 256 and int(blk.max()) == int(blk.min()) + 255
            # four consecutive k of a row are one float4
            q = p[mb * 16:(mb + 1) * 16, kb * 16:(kb + 1) * 16].reshape(16, 4, 4)
            assert torch.equal(q[..., 1:] - q[..., :1], torch.arange(1, 4).expand(16, 4, 3))
            assert bool((q[..., 0] % 4 == 0).all())
    # scalar and tensor forms agree, and the round trip is the identity
    for m, k in ((0, 0), (5, 7), (M - 1, K - 1), (M - 16, 3)):
        assert GO.fm16_index(m, k, K) == int(p[m, k])
    x = torch.randn(M - 3, K)
    assert torch.equal(GO.from_fm16(GO.to_fm16(x), M - 3, K), x)


def test_fm16_matches_the_library_header():
    """the kernels' map (csrc/gemm.h fm16_index) restated independently: same numbers as the formula in the header comment"""
    K = 80
    for m in range(32):
        for k in range(K):
            lib = ((m >> 4) * (K >> 4) + (k >> 4)) * 256 + ((((m & 15) + 16 * ((k & 15) >> 2)) << 2) + (k & 3))
            assert GO.fm16_index(m, k, K) == lib


def test_bf16_rounding_matches_torch():
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 6, (4096,), generator=g).float(),
                   torch.tensor([0.0, -0.0, 1.0, 1.00390625, 1.01171875, -1.00390625, 3.3895314e38, 1e-40])])
    # exact ties in both directions
    ties = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000 - (1 << 32), 0x3F808001, 0x3F807FFF], dtype=torch.int64).to(torch.int32)
    x = torch.cat([x, ties.view(torch.float32)])
    want = x.to(torch.bfloat16)
    assert torch.equal(GO.bf16_round(x), want.float())
    assert torch.equal(GO.bf16_bits(x).to(torch.int16), want.view(torch.int16))


def test_activations_match_torch():
    x = torch.linspace(-9, 9, 4001, dtype=torch.float64)
    assert (GO.activation(x, GO.ACT_GELU_NEW) - F.gelu(x, approximate="tanh")).abs().max() < 1e-14
    assert (GO.activation(x, GO.ACT_GELU_ERF) - F.gelu(x)).abs().max() < 1e-14
    assert torch.equal(GO.activation(x, GO.ACT_RELU), F.relu(x))
    assert torch.equal(GO.activation(x, GO.ACT_NONE), x)
    assert (GO.leaky_relu(x, 0.1) - F.leaky_relu(x, 0.1)).abs().max() < 1e-15
    v = torch.randn(5, 8, dtype=torch.float64)
    assert (GO.geglu(v) - F.gelu(v[:, 1::2]) * v[:, 0::2]).abs().max() < 1e-14


def test_epilogue_order():
    acc = torch.tensor([[-2.0, 3.0]], dtype=torch.float64)
    b = torch.tensor([1.0, -1.0], dtype=torch.float64)
    r = torch.tensor([[10.0, 20.0]], dtype=torch.float64)
    r2 = torch.tensor([[100.0, 200.0]], dtype=torch.float64)
    out = GO.epilogue(acc, b, GO.ACT_RELU, r, r2, 0.5)
    assert torch.equal(out, (F.relu(acc + b) + r + r2) * 0.5)          # [[55, 111]]: the scale covers the residuals, the relu does not
    assert out.tolist() == [[55.0, 111.0]]


@pytest.mark.parametrize("Ci,taps,dil,groups", [(4, 3, 1, 1), (20, 7, 3, 1), (32, 11, 5, 1), (8, 3, 2, 4)])
def test_conv_gather_matches_conv1d(Ci, taps, dil, groups):
    g = torch.Generator().manual_seed(Ci + taps)
    T, Co = 37, 12
    x = torch.randn(T, Ci, generator=g, dtype=torch.float64)
    w = torch.randn(Co, Ci // groups, taps, generator=g, dtype=torch.float64)
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    pad = dil * (taps - 1) // 2
    ref = F.conv1d(x.T.unsqueeze(0), w, b, padding=pad, dilation=dil, groups=groups)[0].T
    xpad = torch.zeros(T + 2 * pad, Ci, dtype=torch.float64)
    xpad[pad:pad + T] = x
    cg_i, cg_o = Ci // groups, Co // groups
    out = torch.empty(T, Co, dtype=torch.float64)
    for gi in range(groups):           # a grouped conv = one GEMM per group (the batch of the positional conv)
        A = GO.conv_gather(xpad[:, gi * cg_i:(gi + 1) * cg_i], taps, dil, T)
        Wt = GO.conv_weight_matrix(w[gi * cg_o:(gi + 1) * cg_o])
        out[:, gi * cg_o:(gi + 1) * cg_o] = A @ Wt.T + b[gi * cg_o:(gi + 1) * cg_o]
    assert (out - ref).abs().max() < 1e-12


@pytest.mark.parametrize("d", [256, 768])
def test_layer_norm_matches_torch(d):
    g = torch.Generator().manual_seed(d)
    x = torch.randn(9, d, generator=g, dtype=torch.float64) * 3 + 1
    bias = torch.randn(d, generator=g, dtype=torch.float64)
    part = torch.randn(4, 9, d, generator=g, dtype=torch.float64)
    w = torch.randn(d, generator=g, dtype=torch.float64)
    b = torch.randn(d, generator=g, dtype=torch.float64)
    v = GO.row_complete(x, bias, part)
    assert (v - (x + bias + part.sum(0))).abs().max() < 1e-13
    assert torch.equal(GO.row_complete(x), x)
    assert (GO.layer_norm(v, w, b) - F.layer_norm(v, (d,), w, b, eps=1e-5)).abs().max() < 1e-12
    mean, rstd = GO.row_stats(v)
    assert ((v - mean[:, None]) * rstd[:, None] - F.layer_norm(v, (d,), eps=1e-5)).abs().max() < 1e-12


def test_att_merge_matches_one_softmax():
    """chunked softmax partials of one attention row merge to the unchunked softmax(s) V"""
    g = torch.Generator().manual_seed(7)
    M, heads, hd, nc, L = 3, 2, 8, 4, 40
    s = torch.randn(M, heads, L, generator=g, dtype=torch.float64) * 8
    V = torch.randn(M, heads, L, hd, generator=g, dtype=torch.float64)
    ref = torch.einsum("mhl,mhld->mhd", torch.softmax(s, dim=-1), V).reshape(M, heads * hd)
    part = torch.zeros(M, heads, nc, hd + 4, dtype=torch.float64)
    for c in range(nc):
        sc, Vc = s[..., c * 10:(c + 1) * 10], V[..., c * 10:(c + 1) * 10, :]
        m = sc.max(dim=-1).values
        p = torch.exp(sc - m.unsqueeze(-1))
        part[:, :, c, :hd] = torch.einsum("mhl,mhld->mhd", p, Vc)
        part[:, :, c, hd] = m
        part[:, :, c, hd + 1] = p.sum(-1)
    assert (GO.att_merge(part, hd) - ref).abs().max() < 1e-12


def test_qkv_scatter_places_rows():
    d, nh, hd, T, max_seq = 8, 2, 4, 3, 10
    acc = torch.arange(6 * 24, dtype=torch.float64).view(6, 24)
    slots, base = torch.tensor([2, 0]), torch.tensor([4, 0, 1])
    kc, vc = torch.full((3, nh, max_seq, hd), -1.0, dtype=torch.float64), torch.full((3, nh, max_seq, hd), -1.0, dtype=torch.float64)
    q = GO.qkv_scatter(acc, None, GO.ACT_NONE, d, nh, hd, T, slots, base, kc, vc)
    assert torch.equal(q, acc[:, :8])
    assert torch.equal(kc[2, 1, 1 + 2], acc[2, 8 + 4:8 + 8])         # entry 0 -> slot 2, base 1, t = 2, head 1
    assert torch.equal(vc[0, 0, 4 + 1], acc[4, 16:20])               # entry 1 -> slot 0, base 4, t = 1, head 0
    assert int((kc != -1).sum()) == 6 * d and bool((kc[1] == -1).all())


def test_gemm_case_struct_matches_the_header_layout():
    """gvc_gemm_case mirrored in ctypes: the size the C compiler gives the header's struct (natural alignment, no packing)"""
    from genvc_amd import _lib
    f = dict((n, getattr(_lib.GemmCase, n)) for n, _ in _lib.GemmCase._fields_)
    got = [f[n].offset for n in ("A", "a_batch_stride", "lda", "att_part", "bias", "kcache", "x_in", "ln_sk")]
    assert got == [16, 48, 96, 136, 176, 280, 312, 368], got         # offsetof() of the header's struct under the x86-64 ABI
    assert C.sizeof(_lib.GemmCase) == 376
