"""tests/attn_oracle.py against torch's own attention (CPU): the restatements the GPU attention mode tests trust are checked here
against an independent implementation, and the ctypes mirror of gvc_attn_case against the header's layout."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_oracle as AO                      # noqa: E402


def _qkv(seed, B, H, Tq, Tk, D, spread=3.0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Tq, D, generator=g, dtype=torch.float64) * spread
    k = torch.randn(B, H, Tk, D, generator=g, dtype=torch.float64)
    v = torch.randn(B, H, Tk, D, generator=g, dtype=torch.float64)
    return q, k, v


def _sdpa(q, k, v, scale, keep):
    """keep bool [B][1 or H][Tq][Tk]"""
    return F.scaled_dot_product_attention(q, k, v, attn_mask=keep, scale=scale)


@pytest.mark.parametrize("base", [0, 7])
def test_causal_matches_sdpa(base):
    B, H, T, D = 2, 3, 9, 16
    q, k, v = _qkv(1 + base, B, H, T, base + T, D)
    limits = AO.causal_limits(torch.tensor([0, 1]), torch.tensor([base, base]) if base else None, T)
    assert limits[0].tolist() == [base + t + 1 for t in range(T)]
    keep = torch.arange(base + T).view(1, 1, 1, -1) < limits.view(B, 1, T, 1)
    if base == 0:          # torch's own causal flag as a second witness
        assert (AO.attend(q, k, v, 0.25, limits) - F.scaled_dot_product_attention(q, k, v, is_causal=True, scale=0.25)).abs().max() < 1e-12
    assert (AO.attend(q, k, v, 0.25, limits) - _sdpa(q, k, v, 0.25, keep)).abs().max() < 1e-12


def test_per_slot_offsets_match_sdpa():
    """slots indirection and per-slot base_len: every stream against its own sdpa call"""
    H, T, D, max_seq = 2, 4, 8, 20
    g = torch.Generator().manual_seed(5)
    kc = torch.randn(5, H, max_seq, D, generator=g, dtype=torch.float64)
    vc = torch.randn(5, H, max_seq, D, generator=g, dtype=torch.float64)
    slots, base = torch.tensor([2, 0, 3]), torch.tensor([6, 99, 0, 11, 99])
    q = torch.randn(3, H, T, D, generator=g, dtype=torch.float64) * 2
    limits = AO.causal_limits(slots, base, T)
    assert limits.tolist() == [[1, 2, 3, 4], [7, 8, 9, 10], [12, 13, 14, 15]]
    got = AO.attend(q, AO.cache_keys(kc, slots), AO.cache_keys(vc, slots), 0.3, limits)
    for b, (slot, bl) in enumerate(((2, 0), (0, 6), (3, 11))):
        n = bl + T
        keep = torch.arange(n).view(1, n) < (bl + torch.arange(T) + 1).view(T, 1)
        ref = _sdpa(q[b:b + 1], kc[slot:slot + 1, :, :n], vc[slot:slot + 1, :, :n], 0.3, keep.view(1, 1, T, n))
        assert (got[b] - ref[0]).abs().max() < 1e-12


@pytest.mark.parametrize("causal", [False, True])
def test_key_padding_mask_matches_sdpa(causal):
    B, H, T, D = 3, 2, 12, 16
    q, k, v = _qkv(9, B, H, T, T, D)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[0, 9:] = False                 # a padding tail
    mask[1, ::2] = False                # alternating keys (the first key among them)
    mask[2, 3:7] = False
    limits = AO.causal_limits(torch.arange(B), None, T) if causal else torch.full((B, T), T)
    keep = mask.view(B, 1, 1, T) & (torch.arange(T).view(1, 1, 1, T) < limits.view(B, 1, T, 1))
    got = AO.attend(q, k, v, 0.25, limits, mask)
    ref = _sdpa(q, k, v, 0.25, keep)
    some = keep.any(dim=-1).expand(B, H, T)          # causal + mask: row 0 of stream 1 sees nothing
    assert (got[some] - ref[some]).abs().max() < 1e-12
    if causal:
        assert not bool(some[1, 0, 0]) and bool((got[1, :, 0] == 0).all())
        assert bool(torch.isnan(AO.attend(q, k, v, 0.25, limits, mask, empty="nan")[1, :, 0]).all())
        assert torch.equal(AO.attend(q, k, v, 0.25, limits, mask, empty="nan")[some], got[some])
    else:
        assert bool(some.all())


@pytest.mark.parametrize("chunks", [1, 2, 4, 8])
def test_merge_of_partials_is_attend(chunks):
    B, H, D = 2, 2, 8
    for nks in ([1, 3, 5], [7, 8, 9], [31, 32, 33, 40]):           # fewer keys than chunks, around a multiple of chunks, several per chunk
        T = len(nks)
        q, k, v = _qkv(chunks + T, B, H, T, max(nks), D, spread=4.0)
        limits = torch.tensor([nks, nks[::-1]])
        o, m, l = AO.partials(q, k, v, 0.35, limits, chunks)
        ref = AO.attend(q, k, v, 0.35, limits)
        assert (AO.merge(o, m, l) - ref).abs().max() < 1e-12
        for b in range(B):
            for t in range(T):
                nk = int(limits[b, t])
                cs = -(-nk // chunks)
                for c in range(chunks):
                    n = min(nk, (c + 1) * cs) - c * cs
                    if n <= 0:
                        assert bool((o[b, :, t, c] == 0).all()) and bool((m[b, :, t, c] == AO.NEG_INF).all()) and bool((l[b, :, t, c] == 0).all())
                    else:               # every chunk's maximum contributes e^0, and a chunk alone is the attention over its keys
                        assert bool((l[b, :, t, c] >= 1).all()) and bool((l[b, :, t, c] <= n + 1e-12).all())
        # one chunk alone: the attention over its own keys
        if chunks == 2:
            cs = -(-nks[-1] // 2)
            lim2 = torch.full((1, 1), nks[-1] - cs)
            alone = AO.attend(q[:1, :, T - 1:T], k[:1, :, cs:nks[-1]], v[:1, :, cs:nks[-1]], 0.35, lim2)
            assert (o[0, :, T - 1, 1] / l[0, :, T - 1, 1].unsqueeze(-1) - alone[0, :, 0]).abs().max() < 1e-12


def test_bf16_cache_is_torch_rounding_and_exact_widening():
    import gemm_oracle as GO
    x = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 7
    r = AO.bf16_cache(x)
    assert torch.equal(r, GO.bf16_round(x))
    assert torch.equal(AO.bf16_cache(r), r) and bool(((r.view(torch.int32) & 0xFFFF) == 0).all())


def test_fused_proj_sums_to_the_projection():
    g = torch.Generator().manual_seed(4)
    H, D = 2, 8
    att = torch.randn(H, D, generator=g, dtype=torch.float64)
    Wp = torch.randn(H * D, H * D, generator=g, dtype=torch.float64)
    part2 = AO.fused_proj(att, Wp)
    assert part2.shape == (H, H * D)
    assert (part2.sum(0) - Wp @ att.reshape(-1)).abs().max() < 1e-13


def test_attn_case_struct_matches_the_header_layout():
    """gvc_attn_case mirrored in ctypes: the offsets the C compiler gives the header's struct (natural alignment, no packing)"""
    from genvc_amd import _lib
    f = dict((n, getattr(_lib.AttnCase, n)) for n, _ in _lib.AttnCase._fields_)
    names = ("q", "k_batch_stride", "q_stride", "scale", "slots", "key_mask", "chunks", "taken", "ran", "seq_len", "max_seq", "nw", "fmask", "ld", "Tq", "E")
    got = [f[n].offset for n in names]
    assert got == [16, 40, 56, 88, 96, 120, 128, 152, 156, 160, 176, 184, 192, 200, 216, 228], got      # offsetof() under the x86-64 ABI
    assert C.sizeof(_lib.AttnCase) == 232
    # the field names and their order are the header's
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "genvc_hip.h")).read()
    body = hdr[hdr.index("typedef struct gvc_attn_case {"):hdr.index("} gvc_attn_case;")]
    import re
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [n for stmt in body.split("{", 1)[1].split(";") for n in re.findall(r"[*\s,]([A-Za-z_]\w*)\s*(?=,|$)", stmt.strip())]
    assert decl == [n for n, _ in _lib.AttnCase._fields_], decl
