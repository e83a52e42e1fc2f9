"""bf16 matrix-core strip GEMM (csrc/gemm_b16.hip, gvc_gemm_probe variant 3) against an fp64 matmul of the bf16-ROUNDED operands:
C = A W^T + bias for the projection shapes of the tiny and the full GPT (reference GPT2Block c_attn / c_proj / c_fc / mlp c_proj,
layers/gpt_inference.py:81-91 through transformers' GPT2Model).  The products of two bf16 values are exact in fp32 and the
accumulation is fp32, so the bar is the one tests/test_gpu_gemm.py holds the fp32 kernels to; a layout or padding mistake is O(1).
Measured maxima on an MI355X: 4.8e-7 (K = 256), 1.9e-6 (K = 1024), 9.5e-6 (K = 4096; 2.9e-6 with the K split) against bars of
7.5e-5 .. 1.3e-3: the hardware's accumulation is well inside the bar, which is kept as it is."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = ((768, 256), (256, 1024), (1024, 4096))


def _probe3(A, W, b, sk_max):
    from genvc_amd import _lib
    out = torch.full((A.shape[0], W.shape[0]), float("nan"), device="cuda")
    us = C.c_float(0)
    _lib.check(_lib.lib().gvc_gemm_probe(3, _lib.ptr(A), _lib.ptr(W), _lib.ptr(b), _lib.ptr(out), A.shape[0], W.shape[0],
                                         A.shape[1], sk_max, 0, C.byref(us), _lib.stream()), "gvc_gemm_probe")
    return out


@pytest.mark.parametrize("M", [1, 17, 129, 145, 437])
def test_bf16_strip_gemm_vs_fp64_of_the_rounded_operands(M):
    """M = 17, 129: one row past a 16-row tile; 145: ten tiles, past a 9-tile m group; 437: several groups.  K split off and up to 8."""
    g = torch.Generator(device="cpu").manual_seed(M)
    for N, K in SHAPES:
        A = torch.randn(M, K, generator=g).cuda()
        W = (torch.randn(N, K, generator=g) * 0.05).cuda()
        b = torch.randn(N, generator=g).cuda()
        Ar, Wr = A.to(torch.bfloat16).double(), W.to(torch.bfloat16).double()
        ref = (Ar @ Wr.T + b.double()).float()
        tol = 2e-5 * (K / 256) ** 0.5 * max(1.0, ref.abs().max().item())
        for sk in (1, 8):
            out = _probe3(A, W, b, sk)
            err = (out - ref).abs().max().item()
            print(f"M={M} N={N} K={K} sk_max={sk}: max err {err:.3e} (bar {tol:.3e})")
            assert err < tol, (M, N, K, sk, err)


@pytest.mark.parametrize("N,K", [(64, 48), (48, 64)], ids=["K_not_32", "N_not_64"])
def test_bf16_strip_probe_rejects_unsupported_shapes(N, K):
    from genvc_amd import _lib
    A = torch.zeros(4, K, device="cuda")
    W = torch.zeros(N, K, device="cuda")
    out = torch.empty(4, N, device="cuda")
    us = C.c_float(0)
    rc = _lib.lib().gvc_gemm_probe(3, _lib.ptr(A), _lib.ptr(W), None, _lib.ptr(out), 4, N, K, 1, 0, C.byref(us), _lib.stream())
    assert rc != 0          # refused, not computed wrong
