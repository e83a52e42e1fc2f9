"""CPU: the teacher-forced oracle helper of the cache-operation tests (tests/cache_ops_oracle.py) against itself -- its one-pass
verification rows equal its own token-by-token rows in every combination of rounding points, the rollback leaves the cache a shorter
run would have left, and a bf16 cache holds bf16-representable rows."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cache_ops_oracle as CO                 # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

TINY = gcfg.TINY_MODEL_ARGS
ROUNDINGS = {"fp32": (False, False, False), "bf16": (True, False, False), "bf16_kv": (True, True, False), "bf16_act": (True, True, True)}


def _case(name, dtype):
    rw, kv, act = ROUNDINGS[name]
    dims = gcfg.gpt_dims(TINY)
    w = {k: v.to(dtype) for k, v in synth.make_weights(5, synth.gpt_weight_spec(dims)).items()}
    if rw:
        w = CO.round_weights(w)
    dims = dict(dims, kv_bf16=kv)
    cond = synth.uniform(7, "cond_latents", (1, 32, dims["d_model"]), 1.0).to(dtype)
    codes = synth.integers(7, "content_codes", (1, 6), 256)
    return w, dims, cond, codes, act


def _bf16_representable(t):
    return torch.equal(t.to(torch.bfloat16).to(t.dtype), t)


@pytest.mark.parametrize("name", list(ROUNDINGS))
def test_one_pass_rows_equal_token_by_token_rows(name):
    """float64, so that the two orders of the same arithmetic differ by ~1e-15 and no value sits that close to a bf16 rounding
    boundary: 9 forced tokens behind a 41-position prefill, mel positions 1..9"""
    w, dims, cond, codes, act = _case(name, torch.float64)
    _, _, cache = CO.prefill(w, dims, cond, codes, act=act)
    assert CO.cache_len(cache) == 32 + 6 + 3
    toks = torch.randint(0, 1024, (9,), generator=torch.Generator().manual_seed(3))
    la, za, ca = CO.forced_rows(w, dims, cache, toks, 1, act=act)
    lb, zb, cb = CO.forced_rows(w, dims, cache, toks, 1, act=act, stepwise=True)
    assert la.shape == (9, dims["num_audio_tokens"]) and za.shape == (9, dims["d_model"])
    assert CO.cache_len(ca) == CO.cache_len(cb) == 41 + 9 and CO.cache_len(cache) == 41          # the input cache is not modified
    assert float((la - lb).abs().max()) < 1e-9 and float((za - zb).abs().max()) < 1e-9
    for (ka, va), (kb, vb) in zip(ca, cb):
        assert float((ka - kb).abs().max()) < 1e-9 and float((va - vb).abs().max()) < 1e-9
        if dims["kv_bf16"]:
            assert _bf16_representable(ka) and _bf16_representable(va) and _bf16_representable(kb) and _bf16_representable(vb)
        else:
            assert not _bf16_representable(ka)
    # the rounding points are live: rounded activations give other rows than unrounded ones
    if act:
        assert float((CO.forced_rows(w, dims, cache, toks, 1, act=False)[1] - za).abs().max()) > 1e-5


def test_float32_passes_agree_to_rounding():
    """the dtype the GPU tests run the oracle in: the two orders agree to float32 rounding where nothing is rounded to bf16"""
    w, dims, cond, codes, _ = _case("fp32", torch.float32)
    _, _, cache = CO.prefill(w, dims, cond, codes)
    toks = torch.randint(0, 1024, (9,), generator=torch.Generator().manual_seed(3))
    la, za, _ = CO.forced_rows(w, dims, cache, toks, 1)
    lb, zb, _ = CO.forced_rows(w, dims, cache, toks, 1, stepwise=True)
    assert float((la - lb).abs().max()) < 2e-5 and float((za - zb).abs().max()) < 2e-5


def test_rollback_then_other_tokens_equals_the_shorter_run():
    """verify 7, drop 3, verify 5 others == forcing the 4 kept tokens and then the 5 (the loop speculative decoding runs)"""
    w, dims, cond, codes, _ = _case("bf16_kv", torch.float64)
    _, _, cache = CO.prefill(w, dims, cond, codes)
    g = torch.Generator().manual_seed(4)
    t1, t2 = torch.randint(0, 1024, (7,), generator=g), torch.randint(0, 1024, (5,), generator=g)
    _, _, c1 = CO.forced_rows(w, dims, cache, t1, 1)
    c1 = CO.rollback(c1, 3)
    assert CO.cache_len(c1) == 41 + 4 and CO.rollback(c1, 0) is c1
    l2, z2, c2 = CO.forced_rows(w, dims, c1, t2, 1 + 4)
    lr, zr, cr = CO.forced_rows(w, dims, cache, torch.cat([t1[:4], t2]), 1)
    assert float((l2 - lr[4:]).abs().max()) < 1e-9 and float((z2 - zr[4:]).abs().max()) < 1e-9
    assert CO.cache_len(c2) == CO.cache_len(cr) == 41 + 9
    assert all(_bf16_representable(k) and _bf16_representable(v) for k, v in c2)


def test_round_weights_rounds_the_block_matrices_and_the_head_only():
    dims = gcfg.gpt_dims(TINY)
    w = synth.make_weights(5, synth.gpt_weight_spec(dims))
    r = CO.round_weights(w)
    for k, v in w.items():
        rounded = k.endswith(CO.BLOCK_MATRICES) or k == "mel_head.weight"
        assert _bf16_representable(r[k]) or not rounded
        assert rounded or r[k] is v
    assert sum(k.endswith(CO.BLOCK_MATRICES) for k in w) == 4 * dims["n_layer"]
