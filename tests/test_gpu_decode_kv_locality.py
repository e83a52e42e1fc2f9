"""The fused attention + c_proj phase (BC) of the one-stream one-launch decode step (csrc/persist_kernel.h) at the edges of its key
slots, bit for bit: logits, latents and the appended K / V rows against tests/golden/decode_kv_locality.npz, recorded from the commit
BEFORE the step's K/V-locality work by scripts/record_decode_kv_locality.py (which runs the cases below) on an MI355X.  Changes to who
computes which unit of BC, to what the loader wave reads and when, or to the diagnostics must leave every bit where it is
(profiles/decode_kv_locality.md).  Also compared at 1e-4 with the launch-per-phase step (GVC_PERSIST=0: other kernels, another summation
order), as tests/test_gpu_decode_variants.py does.

Two layers, d_model 1024, four heads of 256, teacher-forced eager decode steps.  Cached positions S in front of a step (it attends S + 1
keys and appends row S): 36..40 (the shortest prompt), 62..65 (a wave's count of key slots changes at 64), 78..81 (80 keys is the last
fused step, 81 the first on the chunked phases B and C), slots 0, 1 and 2, a cache of 64 rows whose last row (max_seq - 1) the last step
appends, the bf16 KV cache, and launches that find their run flag down."""
import contextlib
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
WIDE2 = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_kv_locality.npz")
SEED = 3

# name: (codes in the prompt, steps, slot, engine) -- the prefill leaves S0 = 32 + codes + 3 cached positions, step j runs at S = S0 + j
CASES = {
    "s36_40": (1, 5, 0, "fp32"),            # S = 36 .. 40
    "s62_65": (27, 4, 2, "fp32"),           # S = 62 .. 65, a slot other than 0
    "s78_81": (43, 4, 1, "fp32"),           # S = 78 .. 81: 79, 80 | 81, 82 keys
    "last_row": (26, 3, 0, "fp32_seq64"),   # S = 61 .. 63 in a cache of 64 rows: the last step appends row max_seq - 1
    "bf16_kv": (27, 4, 1, "bf16_kv"),       # S = 62 .. 65 on the bf16 cache (k_decode_persist<4, 1, 1, 1>)
}
PER_PHASE = ("s36_40", "s62_65", "s78_81", "last_row")      # also run on the launch-per-phase step


@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def prompt(eng, dims, Tc, seed=300):
    cond = synth.uniform(seed, "cond_latents", (1, 32, dims["d_model"]), 1.0)
    codes = synth.integers(seed, "content_codes", (1, Tc), 256)
    return eng.prefix_embeddings(cond.to(DEV), codes.to(DEV).int())


def make_engine(kind, env=None):
    """the switches in `env` are read when the context is created and when its first decode step prepares the one-launch step"""
    from genvc_amd.engine import GptEngine
    dims = gcfg.gpt_dims(WIDE2)
    with environ(env or {}):
        w = synth.make_weights(SEED, synth.gpt_weight_spec(dims), device=DEV)
        eng = GptEngine(dims, max_slots=4, max_rows=2048, max_seq=64 if kind == "fp32_seq64" else None,
                        weight_dtype="bf16_kv" if kind == "bf16_kv" else "fp32")
        eng.bind(w)
        slots = torch.tensor([3], device=DEV, dtype=torch.int32)          # a first step on a slot no case uses
        eng.prefill(slots, prompt(eng, dims, 5), want_outputs=False)
        eng.decode_step(slots, torch.zeros(1, device=DEV, dtype=torch.int32))
        torch.cuda.synchronize()
        eng.health()
    return dims, eng


def kv_row(eng, dims, slot, pos):
    """cached K and V of one position, every layer: [L, 2, H, head_dim] in the cache's element type (bf16 rows as uint16)"""
    from genvc_amd import _lib
    L = _lib.lib()
    L.gvc_gpt_debug_kv_row.restype = C.c_longlong
    L.gvc_gpt_debug_kv_row.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    dt = np.uint16 if eng.weight_dtype == "bf16_kv" else np.float32
    out = np.zeros((dims["n_layer"], 2, dims["n_head"], dims["d_model"] // dims["n_head"]), dtype=dt)
    n = L.gvc_gpt_debug_kv_row(eng._h, slot, pos, out.ctypes.data_as(C.c_void_p))
    assert n == out.nbytes, f"gvc_gpt_debug_kv_row returned {n}"
    return out


def parked(eng, dims, slot):
    from genvc_amd import _lib
    L = _lib.lib()
    L.gvc_gpt_debug_parked.restype = C.c_int
    L.gvc_gpt_debug_parked.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lg = np.zeros(dims["num_audio_tokens"], dtype=np.float32)
    lat = np.zeros(dims["d_model"], dtype=np.float32)
    assert L.gvc_gpt_debug_parked(eng._h, slot, lg.ctypes.data_as(C.c_void_p), lat.ctypes.data_as(C.c_void_p)) == 0
    return lg, lat


def run_case(eng, dims, name, one_launch=True):
    """{name_logits [n, V], name_latent [n, d], name_kv [n, L, 2, H, hd]} of the case's teacher-forced steps"""
    from genvc_amd import _lib
    Tc, n, slot, kind = CASES[name]
    prefix = prompt(eng, dims, Tc)
    S0 = prefix.shape[1] + 1
    toks = synth.integers(5, "toks_" + name, (1, n), 1024)
    slots = torch.tensor([slot], device=DEV, dtype=torch.int32)
    base = eng.one_stream_steps()
    eng.prefill(slots, prefix, want_outputs=False)
    lgs, lats, kvs = [], [], []
    for j in range(n):
        lg, lat = eng.decode_step(slots, toks[:, j].to(DEV).int().contiguous())
        torch.cuda.synchronize()
        lgs.append(lg[0].cpu().numpy().copy())
        lats.append(lat[0].cpu().numpy().copy())
        kvs.append(kv_row(eng, dims, slot, S0 + j))
        assert np.abs(kvs[-1].astype(np.float32)).max() > 0, f"{name}: step {j} appended nothing at row {S0 + j}"
    ran = eng.one_stream_steps() - base
    assert (ran == n) if one_launch else (ran <= 0), f"{name}: {ran} one-launch steps"
    if kind == "fp32_seq64":
        assert S0 + n - 1 == 63, "the last step must append the cache's last row"
        with pytest.raises(_lib.GenvcHipError):      # the step ran and wrote row 63; the position cannot advance: reported, then acknowledged
            eng.health()
        eng.reset(slots)
        torch.cuda.synchronize()
    eng.health()
    return {f"{name}_logits": np.stack(lgs), f"{name}_latent": np.stack(lats), f"{name}_kv": np.stack(kvs)}


def run_flag_down(eng, dims):
    """a generation call that leaves its last token pending, a decode step (flush + step), a second one whose flush launch finds the run
    flag down, then truncate() by zero: ONE launch with the flag down whose outputs nothing overwrites.  Returns what the steps gave and
    what the flag-down launch left where it was."""
    from genvc_amd.engine import sample_params
    prefix = prompt(eng, dims, 13)
    P = prefix.shape[1]
    slots = torch.zeros(1, device=DEV, dtype=torch.int32)
    ids = torch.ones(1, P + 1 + 16, device=DEV, dtype=torch.int32)
    ids[:, P] = dims["start_audio_token"]
    ids_len = torch.full((1,), P + 1, device=DEV, dtype=torch.int32)
    fin = torch.zeros(1, device=DEV, dtype=torch.int32)
    tk = torch.full((1, 4), -1, device=DEV, dtype=torch.int32)
    lats = torch.zeros(1, 4, dims["d_model"], device=DEV)
    eng.prefill(slots, prefix, want_outputs=False)
    eng.generate(slots, ids, ids_len, fin, sample_params(GREEDY, dims["num_audio_tokens"], dims["stop_audio_token"], 0), 0, 4, tk, lats,
                 max_keys=P + 1 + 16)                                   # deferring: the fourth token stays pending
    eng.decode_step(slots, torch.tensor([5], device=DEV, dtype=torch.int32))           # flush (runs) + step: P + 6 positions
    n0 = eng.one_stream_steps()
    lg, lat = eng.decode_step(slots, torch.tensor([9], device=DEV, dtype=torch.int32))  # flush (run flag down) + step: appends row P + 6
    torch.cuda.synchronize()
    eng.health()
    assert eng.one_stream_steps() - n0 == 1, "the launch with its run flag down counted as a step"
    rows = lambda: np.stack([kv_row(eng, dims, 0, P + 5), kv_row(eng, dims, 0, P + 6), kv_row(eng, dims, 0, P + 7)])
    pk0, rows0 = parked(eng, dims, 0), rows()
    eng.truncate(slots, torch.zeros(1, device=DEV, dtype=torch.int32))                # nothing pending: one launch, flag down
    torch.cuda.synchronize()
    eng.health()
    pk1, rows1 = parked(eng, dims, 0), rows()
    assert eng.one_stream_steps() - n0 == 1, "the launch with its run flag down counted as a step"
    assert np.array_equal(pk0[0], pk1[0]) and np.array_equal(pk0[1], pk1[1]), "the launch with its run flag down wrote the parked logits / latent"
    assert np.array_equal(rows0, rows1), "the launch with its run flag down wrote the cache"
    lg2, lat2 = eng.decode_step(slots, torch.tensor([21], device=DEV, dtype=torch.int32))   # appends row P + 7 if the length stood still
    torch.cuda.synchronize()
    eng.health()
    assert np.array_equal(kv_row(eng, dims, 0, P + 6), rows0[1]) and not np.array_equal(kv_row(eng, dims, 0, P + 7), rows0[2]), "the length moved"
    return {"flag_tokens": tk.cpu().numpy(), "flag_latents": lats.cpu().numpy(),
            "flag_logits": np.stack([lg[0].cpu().numpy(), lg2[0].cpu().numpy()]), "flag_latent": np.stack([lat[0].cpu().numpy(), lat2[0].cpu().numpy()]),
            "flag_parked_logits": pk1[0], "flag_parked_latent": pk1[1], "flag_kv": np.stack([rows1[1], kv_row(eng, dims, 0, P + 7)])}


def run_all(kinds=("fp32", "fp32_seq64", "bf16_kv")):
    """every case on the one-launch step: {array name: array}"""
    out = {}
    for kind in kinds:
        torch.cuda.empty_cache()
        dims, eng = make_engine(kind)
        for name, case in CASES.items():
            if case[3] == kind:
                out.update(run_case(eng, dims, name))
        if kind == "fp32":
            out.update(run_flag_down(eng, dims))
        eng.close()
    return out


_GOT = {}


@pytest.fixture(scope="module")
def got():
    if not _GOT:
        _GOT.update(run_all())
    return _GOT


@pytest.fixture(scope="module")
def parent_bits():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", list(CASES) + ["flag"])
def test_bits_of_the_parent_commit(got, parent_bits, name):
    gold = parent_bits
    keys = sorted(k for k in gold if k.startswith(name + "_"))
    assert len(keys) >= 3
    for k in keys:
        a, b = got[k], gold[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{k}: {a.shape} {a.dtype} against {b.shape} {b.dtype}"
        if not np.array_equal(a, b):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            bad = sorted({int(i) for i in np.argwhere(d > 0)[:, 0]}) if a.ndim > 1 else []
            pytest.fail(f"{k} differs from the parent commit's bits: max |diff| {d.max():.3e}, first axis {bad}")


def test_fixture_covers_the_cases(parent_bits):
    gold = parent_bits
    assert {k.rsplit("_", 1)[0] for k in gold if k.endswith("_kv")} == set(CASES) | {"flag"}
    for name, (Tc, n, slot, kind) in CASES.items():
        assert gold[f"{name}_logits"].shape[0] == n and gold[f"{name}_kv"].shape[0] == n
        assert gold[f"{name}_kv"].dtype == (np.uint16 if kind == "bf16_kv" else np.float32)
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_against_the_launch_per_phase_step(got):
    for kind in ("fp32", "fp32_seq64"):
        torch.cuda.empty_cache()
        dims, eng = make_engine(kind, env={"GVC_PERSIST": "0"})
        for name in PER_PHASE:
            if CASES[name][3] != kind:
                continue
            want = run_case(eng, dims, name, one_launch=False)
            for what in ("logits", "latent", "kv"):
                a, b = got[f"{name}_{what}"], want[f"{name}_{what}"]
                print(f"{name}, {what}: max |one-launch - launch-per-phase| = {np.abs(a - b).max():.3e}")
                np.testing.assert_allclose(a, b, atol=1e-4, err_msg=f"{name}: {what} against the launch-per-phase step")
        eng.close()
