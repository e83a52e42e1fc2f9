"""How the one-stream one-launch decode step (csrc/persist_kernel.h) writes its hand-off granules, at the smallest shapes where a change of
that can go wrong, bit for bit: logits, latents and the appended K / V rows against tests/golden/decode_publish_lines.npz, recorded from
the commit BEFORE the whole-line publishes by scripts/record_decode_publish_lines.py (which runs the cases below) on an MI355X.  Which
wave stores a granule, with how many lanes and through which staging array may change; the granule's index, tag and value may not
(profiles/decode_publish_lines.md).  tests/test_gpu_decode_kv_locality.py holds d_model 1024 on the XCD-local fused path to the same
standard; here:

  * d_model 256, 512 and 768, two layers: a workgroup owns 3, 6 and 9 rows of c_attn (sub-line, unaligned runs of granules), 1, 2 and 3
    rows of the projections, and its weight segments are no multiples of a 16 KiB fill (the last fill of a segment is partial);
  * 1, 2 and 4 heads of 256 (the fused attention + c_proj phase writes H, 2 H, 4 H granules per workgroup), 3 heads of 256 and 4 of 128
    (always on the chunked phases B and C);
  * contexts on both sides of the 80-key switch between the fused phase and the chunked ones, one step on either side of it;
  * d_model 1024 without the XCD-local MLP hand-off (GVC_PERSIST_XCD=0: the device-wide phases C, D and E);
  * bf16 weights and the bf16 KV cache at d_model 512 and 1024;
  * the vocabulary of 1026 (256 workgroups x 4 rows and 2 remainder rows) throughout, slots 0, 1 and 2;
  * a launch that finds its run flag down: no granule, no weight load, and the next step's bits where they were."""
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
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_publish_lines.npz")
SEED = 3

# engine: (d_model, heads, weight_dtype, environment while the context and its one-launch step are prepared)
ENGINES = {
    "d256_h1": (256, 1, "fp32", {}),
    "d512_h2": (512, 2, "fp32", {}),
    "d512_h4": (512, 4, "fp32", {}),                        # heads of 128: chunked phases at every context
    "d768_h3": (768, 3, "fp32", {}),                        # 256 workgroups are no multiple of 3 heads: chunked phases at every context
    "d512_bf16": (512, 2, "bf16", {}),
    "d512_bf16kv": (512, 2, "bf16_kv", {}),
    "d1024_noxl": (1024, 4, "fp32", {"GVC_PERSIST_XCD": "0"}),
    "d1024_bf16": (1024, 4, "bf16", {}),
}
# case: (engine, codes in the prompt, steps, slot) -- the prefill leaves S0 = 32 + codes + 3 cached positions, step j attends S0 + j + 1 keys
CASES = {
    "d256_h1_switch": ("d256_h1", 43, 4, 0),                # 79, 80 | 81, 82 keys
    "d512_h2_switch": ("d512_h2", 43, 4, 1),
    "d512_h2_short": ("d512_h2", 1, 3, 2),                  # 37 .. 39 keys, the third slot
    "d512_h4_chunked": ("d512_h4", 27, 3, 2),
    "d768_h3_chunked": ("d768_h3", 43, 4, 1),
    "d512_bf16_switch": ("d512_bf16", 43, 4, 0),
    "d512_bf16kv_switch": ("d512_bf16kv", 43, 4, 2),
    "d1024_noxl_switch": ("d1024_noxl", 43, 4, 1),
    "d1024_bf16_switch": ("d1024_bf16", 43, 4, 2),
}
FLAG_ENGINE = "d512_h2"


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


def make_engine(name):
    from genvc_amd.engine import GptEngine
    d, H, wdt, env = ENGINES[name]
    dims = gcfg.gpt_dims(dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2, gpt_n_model_channels=d, gpt_n_heads=H))
    assert dims["num_audio_tokens"] == 1026
    with environ(env):
        w = synth.make_weights(SEED, synth.gpt_weight_spec(dims), device=DEV)
        eng = GptEngine(dims, max_slots=4, max_rows=2048, weight_dtype=wdt)
        eng.bind(w)
        slots = torch.tensor([3], device=DEV, dtype=torch.int32)          # a first step on a slot no case uses: prepares the one-launch step
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


def run_case(eng, dims, name):
    """{name_logits [n, V], name_latent [n, d], name_kv [n, L, 2, H, hd]} of the case's teacher-forced steps"""
    _, Tc, n, slot = CASES[name]
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
    assert ran == n, f"{name}: {ran} one-launch steps of {n}"
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


def run_engine(name):
    """every case of one engine: {array name: array}"""
    torch.cuda.empty_cache()
    out = {}
    dims, eng = make_engine(name)
    for case, spec in CASES.items():
        if spec[0] == name:
            out.update(run_case(eng, dims, case))
    if name == FLAG_ENGINE:
        out.update(run_flag_down(eng, dims))
    eng.close()
    return out


def run_all():
    out = {}
    for name in ENGINES:
        out.update(run_engine(name))
    return out


_GOT = {}


def got_of(engine):
    if engine not in _GOT:
        _GOT[engine] = run_engine(engine)
    return _GOT[engine]


@pytest.fixture(scope="module")
def parent_bits():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("name", list(CASES) + ["flag"])
def test_bits_of_the_parent_commit(parent_bits, name):
    gold = parent_bits
    got = got_of(FLAG_ENGINE if name == "flag" else CASES[name][0])
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
    for name, (engine, Tc, n, slot) in CASES.items():
        d, H, wdt, _ = ENGINES[engine]
        assert gold[f"{name}_logits"].shape == (n, 1026) and gold[f"{name}_latent"].shape == (n, d)
        assert gold[f"{name}_kv"].shape == (n, 2, 2, H, d // H)
        assert gold[f"{name}_kv"].dtype == (np.uint16 if wdt == "bf16_kv" else np.float32)
    assert {spec[3] for spec in CASES.values()} == {0, 1, 2}
    assert os.path.getsize(GOLDEN) < 1 << 20
