"""The one-stream one-launch decode step (csrc/persist_kernel.h) in the variants the launcher chooses between: production and stamping
(GVC_PERSIST_STAMPS, a template parameter of the kernel), the fused and the chunked attention phases on either side of 80 keys, a launch
that finds its run flag down, and the d_model 256 instantiation.  Two layers and short contexts throughout; every comparison between two
builds of the SAME arithmetic is bit-exact, the launch-per-phase step (GVC_PERSIST=0: other kernels, another summation order) is compared at
the 1e-4 the GPT tests use for either path against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from genvc_amd import config as gcfg
from genvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GREEDY = dict(gcfg.DEFAULT_SAMPLING, top_k=1)
WIDE2 = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2)          # d = 1024, H = 4, head_dim 256, L = 2: the headline's instantiation
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_boundary_79_80_81.npz")


def engine(monkeypatch, margs, seed, env=None):
    """(dims, weights, engine); `env` is set while the context is created AND while its first decode step prepares the one-launch
    step (both read their switches then), and removed afterwards"""
    from genvc_amd.engine import GptEngine
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    dims = gcfg.gpt_dims(margs)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims), device=DEV)
    eng = GptEngine(dims, max_slots=4, max_rows=2048)
    eng.bind(w)
    slots = torch.tensor([3], device=DEV, dtype=torch.int32)          # a first step on a slot no test uses: prepares the decode path
    eng.prefill(slots, prompt(eng, dims, 5), want_outputs=False)
    eng.decode_step(slots, torch.zeros(1, device=DEV, dtype=torch.int32))
    torch.cuda.synchronize()
    eng.health()
    for k in (env or {}):
        monkeypatch.delenv(k)
    return dims, w, eng


def prompt(eng, dims, Tc, seed=300):
    cond = synth.uniform(seed, "cond_latents", (1, 32, dims["d_model"]), 1.0)
    codes = synth.integers(seed, "content_codes", (1, Tc), 256)
    return eng.prefix_embeddings(cond.to(DEV), codes.to(DEV).int())


def kv_row(eng, dims, slot, pos):
    """cached K and V of one position, every layer: [L, 2, H, head_dim] (csrc/gpt.hip: gvc_gpt_debug_kv_row)"""
    from genvc_amd import _lib
    L = _lib.lib()
    L.gvc_gpt_debug_kv_row.restype = C.c_longlong
    L.gvc_gpt_debug_kv_row.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    out = np.zeros((dims["n_layer"], 2, dims["n_head"], dims["d_model"] // dims["n_head"]), dtype=np.float32)
    n = L.gvc_gpt_debug_kv_row(eng._h, slot, pos, out.ctypes.data_as(C.c_void_p))
    assert n == out.nbytes, f"gvc_gpt_debug_kv_row returned {n}"
    return out


def parked(eng, dims, slot):
    """(logits, latent) parked for a slot between calls (csrc/gpt.hip: gvc_gpt_debug_parked)"""
    from genvc_amd import _lib
    L = _lib.lib()
    L.gvc_gpt_debug_parked.restype = C.c_int
    L.gvc_gpt_debug_parked.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lg = np.zeros(dims["num_audio_tokens"], dtype=np.float32)
    lat = np.zeros(dims["d_model"], dtype=np.float32)
    assert L.gvc_gpt_debug_parked(eng._h, slot, lg.ctypes.data_as(C.c_void_p), lat.ctypes.data_as(C.c_void_p)) == 0
    return lg, lat


def stamp_words(eng, dims):
    """the stamp buffer of the one-launch step, or None when the context has none (the production variant)"""
    from genvc_amd import _lib
    L = _lib.lib()
    L.gvc_gpt_debug_stamps.restype = C.c_int
    L.gvc_gpt_debug_stamps.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    hb = np.zeros(20 * (dims["n_layer"] + 2) + 10 * 256 + 8 * 256, dtype=np.uint64)
    n = L.gvc_gpt_debug_stamps(eng._h, hb.ctypes.data_as(C.c_void_p), -1)
    return hb if n > 0 else None


def teacher_forced(eng, dims, prefix, toks, slot=0, rows=False):
    """prefill, then one decode step per token: [(logits, latent)] per step, and with rows=True the K/V each step appended"""
    slots = torch.tensor([slot], device=DEV, dtype=torch.int32)
    eng.prefill(slots, prefix, want_outputs=False)
    P = prefix.shape[1]
    out, kv = [], []
    for j in range(toks.shape[1]):
        lg, lat = eng.decode_step(slots, toks[:, j].to(DEV).int().contiguous())
        torch.cuda.synchronize()
        out.append((lg.cpu().clone(), lat.cpu().clone()))
        if rows:
            kv.append(kv_row(eng, dims, slot, P + 1 + j))        # the prefill left P + 1 positions: step j appends position P + 1 + j
    eng.health()
    return out, kv


def test_production_and_stamping_variants_agree(monkeypatch):
    """logits, latent and the appended K/V of eight consecutive steps, then a generation call of eight (whose first launch leaves at the
    run flag), are bit-identical between the production variant and the stamping one; the stamping context has stamps, the other none"""
    torch.cuda.empty_cache()
    dims, w, prod = engine(monkeypatch, WIDE2, 3)
    _, _, stmp = engine(monkeypatch, WIDE2, 3, env={"GVC_PERSIST_STAMPS": "1"})
    toks = synth.integers(5, "toks", (1, 8), 1024)
    res = []
    for eng in (prod, stmp):
        base = eng.one_stream_steps()
        out, kv = teacher_forced(eng, dims, prompt(eng, dims, 13), toks, rows=True)
        assert eng.one_stream_steps() - base == 8, "not on the one-launch step"
        res.append((out, kv))
    for j in range(8):
        assert torch.equal(res[0][0][j][0], res[1][0][j][0]), f"logits of step {j}"
        assert torch.equal(res[0][0][j][1], res[1][0][j][1]), f"latent of step {j}"
        assert np.array_equal(res[0][1][j], res[1][1][j]), f"appended K/V of step {j}"
        assert np.abs(res[0][1][j]).max() > 0, f"step {j} appended nothing"
    assert stamp_words(prod, dims) is None, "the production context carries a stamp buffer"
    st = stamp_words(stmp, dims)
    assert st is not None and st[: 20 * dims["n_layer"]].max() > 0, "the stamping variant wrote no stamps"
    # a generation call on top: [early exit, sample] then seven executed steps
    from genvc_amd.engine import sample_params
    gen = []
    for eng in (prod, stmp):
        prefix = prompt(eng, dims, 13)
        P = prefix.shape[1]
        slots = torch.zeros(1, device=DEV, dtype=torch.int32)
        ids = torch.ones(1, P + 1 + 16, device=DEV, dtype=torch.int32)
        ids[:, P] = dims["start_audio_token"]
        ids_len = torch.full((1,), P + 1, device=DEV, dtype=torch.int32)
        fin = torch.zeros(1, device=DEV, dtype=torch.int32)
        tk = torch.full((1, 8), -1, device=DEV, dtype=torch.int32)
        lats = torch.zeros(1, 8, dims["d_model"], device=DEV)
        eng.prefill(slots, prefix, want_outputs=False)
        eng.generate(slots, ids, ids_len, fin, sample_params(GREEDY, dims["num_audio_tokens"], dims["stop_audio_token"], 0), 0, 8, tk, lats,
                     max_keys=P + 1 + 16)
        torch.cuda.synchronize()
        eng.health()
        assert eng.decode_variant() == 3
        gen.append((tk.cpu(), lats.cpu()))
    assert torch.equal(gen[0][0], gen[1][0]) and torch.equal(gen[0][1], gen[1][1])
    prod.close()
    stmp.close()


def boundary_run(eng, dims):
    """teacher-forced steps over contexts of 77 .. 84 keys; returns {keys: (logits, latent)}"""
    P0 = prompt(eng, dims, 13).shape[1]
    Tc = 13 + (75 - P0)                     # prefix of 75 rows: 76 cached positions after the prefill, the first step attends 77 keys
    prefix = prompt(eng, dims, Tc)
    assert prefix.shape[1] == 75
    toks = synth.integers(7, "toks", (1, 8), 1024)
    out, _ = teacher_forced(eng, dims, prefix, toks)
    return {77 + j: out[j] for j in range(8)}


def test_fused_unfused_boundary(monkeypatch):
    """steps at 79, 80 (the last fused one) and 81 keys (the first on the chunked phases B and C): bit-identical to what the kernel gave
    before its scalar live ranges were shortened (tests/golden, recorded from the parent commit's library on an MI355X), and within 1e-4
    of the launch-per-phase step"""
    torch.cuda.empty_cache()
    dims, w, one = engine(monkeypatch, WIDE2, 3)
    base = one.one_stream_steps()
    got = boundary_run(one, dims)
    assert one.one_stream_steps() - base == 8, "not on the one-launch step"
    one.close()
    _, _, lpp = engine(monkeypatch, WIDE2, 3, env={"GVC_PERSIST": "0"})
    want = boundary_run(lpp, dims)
    assert lpp.one_stream_steps() <= 0, "GVC_PERSIST=0 still ran the one-launch step"
    lpp.close()
    gold = np.load(GOLDEN)
    for keys in (79, 80, 81):
        for i, what in enumerate(("logits", "latent")):
            a, b = got[keys][i].numpy(), want[keys][i].numpy()
            print(f"{keys} keys, {what}: max |one-launch - launch-per-phase| = {np.abs(a - b).max():.3e}")
            np.testing.assert_allclose(a, b, atol=1e-4, err_msg=f"{what} at {keys} keys vs the launch-per-phase step")
            assert np.array_equal(a, gold[f"{what}_{keys}"]), f"{what} at {keys} keys differs from the parent commit's bits"


def test_run_flag_down_touches_nothing(monkeypatch):
    """A decode step behind a deferring generation call flushes the slot's pending token with a conditional launch; a SECOND decode step
    finds nothing pending, so its flush launch leaves at the run flag.  That launch must not count as a step, must leave the cache rows,
    the length and the parked logits / latent alone, and the step behind it must give what a context gives that never defers
    (GVC_DEFER_DECODE=0: no conditional launch at all) -- bit for bit, as must the step after that.  The outputs of those two
    launches are overwritten by the step behind them, so a third one follows whose outputs nothing overwrites (truncate by zero): the
    parked logits and latent, the cache and the step count are read directly before and after it.  (The generation call in front
    starts with a launch that leaves at the flag too, between the prefill's parked logits and the sampler that reads them: its tokens and
    latents are compared as well.)"""
    from genvc_amd.engine import sample_params
    torch.cuda.empty_cache()
    dims, w, d = engine(monkeypatch, WIDE2, 3)
    _, _, e = engine(monkeypatch, WIDE2, 3, env={"GVC_DEFER_DECODE": "0"})
    res = []
    for eng in (d, e):
        prefix = prompt(eng, dims, 13)
        P = prefix.shape[1]
        slots = torch.zeros(1, device=DEV, dtype=torch.int32)
        ids = torch.ones(1, P + 1 + 32, device=DEV, dtype=torch.int32)
        ids[:, P] = dims["start_audio_token"]
        ids_len = torch.full((1,), P + 1, device=DEV, dtype=torch.int32)
        fin = torch.zeros(1, device=DEV, dtype=torch.int32)
        tk = torch.full((1, 16), -1, device=DEV, dtype=torch.int32)
        lats = torch.zeros(1, 16, dims["d_model"], device=DEV)
        sp = sample_params(GREEDY, dims["num_audio_tokens"], dims["stop_audio_token"], 0)
        eng.prefill(slots, prefix, want_outputs=False)
        eng.generate(slots, ids, ids_len, fin, sp, 0, 8, tk, lats, max_keys=P + 1 + 32)        # deferring: the eighth token stays pending
        tok = torch.tensor([5], device=DEV, dtype=torch.int32)
        eng.decode_step(slots, tok)                       # flush (runs) + step: P + 10 positions cached now
        n0 = eng.one_stream_steps()
        before = [kv_row(eng, dims, 0, P + 9), kv_row(eng, dims, 0, P + 10), kv_row(eng, dims, 0, P + 11)]
        lg, lat = eng.decode_step(slots, torch.tensor([9], device=DEV, dtype=torch.int32))      # flush (run flag down) + step
        torch.cuda.synchronize()
        eng.health()
        assert eng.one_stream_steps() - n0 == 1, "the launch with its run flag down counted as a step"
        after = [kv_row(eng, dims, 0, P + 9), kv_row(eng, dims, 0, P + 10), kv_row(eng, dims, 0, P + 11)]
        assert np.array_equal(before[0], after[0]), "a cached row changed"
        assert np.abs(after[1]).max() > 0, "the step appended nothing at its position"
        assert np.array_equal(before[2], after[2]), "the position behind the appended one was written (the length moved twice)"
        lg3, lat3 = eng.decode_step(slots, torch.tensor([17], device=DEV, dtype=torch.int32))   # once more: flag down again, then a step
        torch.cuda.synchronize()
        eng.health()
        assert eng.one_stream_steps() - n0 == 2
        # A launch with the flag down whose outputs nothing overwrites: truncate() by zero positions settles the slot first (nothing is
        # pending: in the deferring context that is ONE conditional launch aimed at the slot's parked rows, in the other nothing at
        # all) and then leaves the length where it is.  Parked logits and latent, the cache and the step count are read on either side.
        pk0, rows0 = parked(eng, dims, 0), [kv_row(eng, dims, 0, P + 11), kv_row(eng, dims, 0, P + 12)]
        eng.truncate(slots, torch.zeros(1, device=DEV, dtype=torch.int32))
        torch.cuda.synchronize()
        eng.health()
        pk1, rows1 = parked(eng, dims, 0), [kv_row(eng, dims, 0, P + 11), kv_row(eng, dims, 0, P + 12)]
        assert eng.one_stream_steps() - n0 == 2, "the launch with its run flag down counted as a step"
        assert np.array_equal(pk0[0], pk1[0]), "the launch with its run flag down wrote the parked logits"
        assert np.array_equal(pk0[1], pk1[1]), "the launch with its run flag down wrote the parked latent"
        assert np.array_equal(rows0[0], rows1[0]) and np.array_equal(rows0[1], rows1[1]), "the launch with its run flag down wrote the cache"
        r13 = kv_row(eng, dims, 0, P + 13)
        lg4, lat4 = eng.decode_step(slots, torch.tensor([21], device=DEV, dtype=torch.int32))   # appends at P + 12 if the length stood still
        torch.cuda.synchronize()
        eng.health()
        assert not np.array_equal(kv_row(eng, dims, 0, P + 12), rows0[1]) and np.array_equal(kv_row(eng, dims, 0, P + 13), r13), "the length moved"
        res.append(dict(logits=lg.cpu(), latent=lat.cpu(), row=after[1], logits3=lg3.cpu(), latent3=lat3.cpu(), row3=rows0[0],
                        logits4=lg4.cpu(), latent4=lat4.cpu(), row4=kv_row(eng, dims, 0, P + 12),
                        tokens=tk.cpu(), latents=lats.cpu(), ids=ids.cpu(), ids_len=ids_len.cpu()))
    for k in res[0]:
        a, b = res[0][k], res[1][k]
        assert (np.array_equal(a, b) if isinstance(a, np.ndarray) else torch.equal(a, b)), f"{k} differs from the context that never defers"
    d.close()
    e.close()


def test_small_d_model_takes_the_unfused_path(monkeypatch):
    """d_model 256 (four heads of 64: no fused attention phase at any context length): the one-launch step against the launch-per-phase
    step, and a second instantiation of the per-phase scalar handling"""
    torch.cuda.empty_cache()
    toks = synth.integers(11, "toks", (1, 6), 1024)
    outs = []
    for env in (None, {"GVC_PERSIST": "0"}):
        dims, w, eng = engine(monkeypatch, gcfg.TINY_MODEL_ARGS, 23, env=env)
        base = eng.one_stream_steps()
        out, _ = teacher_forced(eng, dims, prompt(eng, dims, 21, seed=23), toks)
        ran = eng.one_stream_steps() - base
        assert (ran == 6) if env is None else (ran <= 0), f"{ran} one-launch steps with {env}"
        outs.append(out)
        eng.close()
    for j in range(6):
        for i, what in enumerate(("logits", "latent")):
            a, b = outs[0][j][i].numpy(), outs[1][j][i].numpy()
            print(f"step {j}, {what}: max |one-launch - launch-per-phase| = {np.abs(a - b).max():.3e}")
            np.testing.assert_allclose(a, b, atol=1e-4, err_msg=f"{what} of step {j}")
