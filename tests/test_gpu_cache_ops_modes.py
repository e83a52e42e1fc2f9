"""GPU: the primitives that continue or rearrange an existing KV cache, in every storage mode of the GPT context (`weight_dtype` "fp32",
"bf16", "bf16_kv", "bf16_act", "bf16_mfma"; include/genvc_hip.h): gvc_gpt_verify / gvc_gpt_truncate, gvc_gpt_kv_fanout, the span copies
of the beam step, and a prefill onto a cached prefix.

References.  Every verification pass is compared with (1) the same tokens fed one gvc_gpt_decode_step at a time to fanned-out copies of
the slots and (2) the CPU oracle, teacher-forced per slot (tests/cache_ops_oracle.py), with the rounding points of the path the call took:
  * weights rounded to bf16 in every mode but "fp32"; k / v rounded into the cache from "bf16_kv" on;
  * activations rounded (oracle `act_bf16`) where `act_rows` says so: a "bf16_act" context rounds them on the one-launch rows step only
    (d = 1024, 2..16 rows) -- past 16 rows, with one row, and at d = 256 / 512 it runs the fp32-activation paths and is compared with
    fp32 activations; a "bf16_mfma" context rounds them in every pass of two or more rows (rows step or bf16 strip GEMMs; its prefill
    too), a one-row step runs the one-stream step or the GEMV step with fp32 activations.
  Where the verification pass and its sequential comparator round at different points (a 17-row pass against one-row steps), the two are
  not the same function: the sequential steps are then held to the oracle with THEIR rounding points instead of to the pass.

Tolerances (the project's, none new): "fp32" / "bf16" 1e-4 on logits and latents (test_gpu_assisted.TOL, the bf16 rule of test_gpu_gpt);
"bf16_kv" 2e-3 (test_bf16_weight_mode_matches_oracle_on_rounded_weights); "bf16_act" / "bf16_mfma" the yardstick of
test_gpu_round6.test_rows_step_bf16_activations_vs_oracle and test_gpu_bf16_mfma with their factors: the latents' deviation against
the oracle's own reproducibility ball -- median <= 3 x + 1e-4, 99.9 % quantile <= 3 x + 1e-3.  The ball here is the oracle's float64
run against its float32 run with the same rounding points (`genvc_oracle._bf16` rounds in the run's own dtype for this purpose).
Those two tests move the conditioning input by 2e-7 relative instead, which measures the same thing on their shapes but not on these:
a bf16_mfma prefill rounds its input rows to bf16 before anything else, a 2e-7 step changes such a rounding with probability ~5e-5
per element, and behind a prefill of 36..100 rows of d = 256 it often changes none -- the "perturbed" run is then bit-identical to
the reference (measured: median 0.0) and no implementation but a bit-exact one could meet 3 x 0.  Float rounding in every operation
of the float32 run, as on the device, does not vanish that way.  Every case prints its deviations and bounds; DESIGN.md section 4.25
records them.

Everything is teacher-forced (seeded tokens), so no margin screening is needed."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cache_ops_oracle as CO                 # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026
MODELS = {"tiny": gcfg.TINY_MODEL_ARGS,                                                           # d 256, head_dim 64
          "full2": dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2),                                   # d 1024, head_dim 256
          "d512": dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2, gpt_n_model_channels=512)}          # d 512, head_dim 128
MODES = ["fp32", "bf16", "bf16_kv", "bf16_act", "bf16_mfma"]
ACT_MODES = ("bf16_act", "bf16_mfma")
TOL = {"fp32": 1e-4, "bf16": 1e-4, "bf16_kv": 2e-3}
W_SEED = 5
MAX_SLOTS = 16

_engines, _weights, _prefills = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng in _engines.values():
        eng.close()
    _engines.clear()
    _weights.clear()
    _prefills.clear()
    torch.cuda.empty_cache()


def sl(*i):
    return torch.tensor(i, device=DEV, dtype=torch.int32)


def model_weights(model):
    """(dims, device weights, CPU weights, CPU weights rounded as a bf16 context rounds them), built once per model"""
    if model not in _weights:
        dims = gcfg.gpt_dims(MODELS[model])
        w = synth.make_weights(W_SEED, synth.gpt_weight_spec(dims), device=DEV)
        wc = {k: v.cpu() for k, v in w.items()}
        _weights[model] = (dims, w, wc, CO.round_weights(wc))
    return _weights[model]


def engine(model, mode, max_seq=None):
    """one context per (model, mode, max_seq) for the module, every slot reset"""
    from genvc_amd.engine import GptEngine
    key = (model, mode, max_seq)
    dims, w, _, _ = model_weights(model)
    if key not in _engines:
        eng = GptEngine(dims, max_slots=MAX_SLOTS, max_rows=2048, max_seq=max_seq, weight_dtype=mode)
        eng.bind(w)
        _engines[key] = eng
    eng = _engines[key]
    eng.reset(torch.arange(MAX_SLOTS, device=DEV, dtype=torch.int32))
    return eng, dims


def oracle_setup(model, mode, double=False):
    dims, _, wc, wr = model_weights(model)
    w = wc if mode == "fp32" else wr
    if double:
        key = (model, mode == "fp32", "f64")
        if key not in _weights:
            _weights[key] = f64(w)
        w = _weights[key]
    return w, dict(dims, kv_bf16=mode in ("bf16_kv",) + ACT_MODES)


def act_rows(model, mode, rows):
    """does a pass of `rows` rows that continue cached slots round its activations?  (module docstring; csrc/gpt.hip: run_rows)"""
    if mode == "bf16_act":
        return model == "full2" and 2 <= rows <= 16
    return mode == "bf16_mfma" and rows >= 2


def variant_of(model, rows):
    """gvc_gpt_decode_variant after a verification pass: 5 = the one-launch rows step (d 1024, 2..16 rows), 4 = the GEMM path"""
    return 5 if model == "full2" and 2 <= rows <= 16 else 4


def slot_inputs(model, seed, tc, B=1):
    d = MODELS[model]["gpt_n_model_channels"]
    return synth.uniform(seed, "cond_latents", (B, 32, d), 1.0), synth.integers(seed, "content_codes", (B, tc), 256)


def f64(w):
    return {k: v.double() for k, v in w.items()}


def base_of(tc):
    """cached positions behind a prefill of tc content codes: 32 conditioning rows, <s> codes </s>, the start token"""
    return 32 + tc + 2 + 1


def device_prefill(eng, model, slot, seed, tc):
    cond, codes = slot_inputs(model, seed, tc)
    eng.prefill(sl(slot), eng.prefix_embeddings(cond.to(DEV), codes.to(DEV).int()), want_outputs=False)


def oracle_prefill(model, mode, seed, tc, double):
    """(latent, logits, cache) of the oracle's prefill of one slot, shared by the cases of the module (read-only)"""
    act = mode == "bf16_mfma"                     # the prefill of a bf16_mfma context runs on the bf16 strip GEMMs
    key = (model, mode == "fp32", mode in ("bf16_kv",) + ACT_MODES, act, seed, tc, double)
    if key not in _prefills:
        w, dims = oracle_setup(model, mode, double)
        cond, codes = slot_inputs(model, seed, tc)
        _prefills[key] = CO.prefill(w, dims, cond.double() if double else cond, codes, act=act)
    return _prefills[key]


class Twin:
    """one slot of the oracle (float32) and, in the activation-rounding modes, the same slot in float64: the difference of the two is
    the yardstick of those modes"""

    def __init__(self, model, mode, seed, tc):
        self.dims = oracle_setup(model, mode)[1]
        self.ws = [oracle_setup(model, mode, dbl)[0] for dbl in ([False, True] if mode in ACT_MODES else [False])]
        self.caches = [oracle_prefill(model, mode, seed, tc, dbl)[2] for dbl in ([False, True] if mode in ACT_MODES else [False])]
        self.j = 1

    def fork(self):
        t = copy.copy(self)
        t.caches = list(self.caches)
        return t

    def rows(self, toks, act):
        """-> (logits [T, V], latents [T, d], |float64 latents - latents| or None); the slot grows by T"""
        outs = []
        for i, c in enumerate(self.caches):
            lg, z, self.caches[i] = CO.forced_rows(self.ws[i], self.dims, c, toks, self.j, act=act)
            outs.append((lg, z))
        self.j += int(torch.as_tensor(toks).numel())
        return outs[0][0], outs[0][1], ((outs[1][1].float() - outs[0][1]).abs() if len(outs) > 1 else None)

    def drop(self, n):
        self.caches = [CO.rollback(c, n) for c in self.caches]
        self.j -= n


def _q(t, p):
    return float(torch.quantile(t.flatten().double(), p))


class Check:
    """collects (device rows, reference rows, yardstick) of one comparison of a case and asserts the mode's rule over all of them"""

    def __init__(self, what, mode):
        self.what, self.mode = what, mode
        self.dl, self.dz, self.ball = [], [], []

    def add(self, got_l, got_z, ref_l, ref_z, ball=None):
        self.dl.append((got_l.detach().cpu().float() - ref_l.detach().cpu().float()).abs().flatten())
        self.dz.append((got_z.detach().cpu().float() - ref_z.detach().cpu().float()).abs().flatten())
        if ball is not None:
            self.ball.append(ball.flatten())

    def finish(self):
        dl, dz = torch.cat(self.dl), torch.cat(self.dz)
        if self.mode not in ACT_MODES:
            tol = TOL[self.mode]
            print(f"  {self.what}: logits err {float(dl.max()):.3e}, latent err {float(dz.max()):.3e} (tolerance {tol:.0e})")
            assert float(dl.max()) < tol and float(dz.max()) < tol, (self.what, float(dl.max()), float(dz.max()), tol)
            return
        ball = torch.cat(self.ball)
        assert ball.numel() == dz.numel()
        m, y, m9, y9 = _q(dz, 0.5), _q(ball, 0.5), _q(dz, 0.999), _q(ball, 0.999)
        print(f"  {self.what}: latent median {m:.3e} (bound 3 x {y:.3e} + 1e-4), 99.9 % {m9:.3e} (bound 3 x {y9:.3e} + 1e-3); "
              f"logits max {float(dl.max()):.3e} (printed only)")
        assert m <= 3.0 * y + 1e-4, (self.what, m, y)
        assert m9 <= 3.0 * y9 + 1e-3, (self.what, m9, y9)


def rows_step_chunks(rows, keys):
    """key chunks per (row, head) of the one-launch rows step (csrc/gpt.hip: launch_rows_persist, split1 / split2; the kernel picks
    them from the longest context among the rows of the call)"""
    s1, s2 = (80, 160) if rows <= 8 else (128, 288)
    return 4 if keys > s2 else (2 if keys > s1 else 1)


# ---- 1. verify and truncate: modes x row regimes x context regimes ---------------------------------------------------------------
# name: (model, B, T, content codes per slot, what the case is for).  The regime keys are asserted from the computed key counts:
#   chunks    key chunks of the rows step;  straddle: the T rows of the longest slot end on both sides of this many keys
#   cross     the T rows of the (only) slot pass this many keys: the one-stream comparator's 128-key switch
#   past      the longest slot ends past this many keys;  ragged: a slot at the shortest base next to one past the 4-chunk threshold
#   tile      launch_attention_tile accepts the shape (T >= 16, B * ceil(T / 16) >= 12);  max_seq: the context's capacity
VERIFY = {
    "full2_2x4_one_chunk": ("full2", 2, 4, (1, 20), dict(chunks=1)),
    "full2_2x4_across_80": ("full2", 2, 4, (1, 43), dict(chunks=2, straddle=80)),
    "full2_2x4_across_160_ragged": ("full2", 2, 4, (1, 123), dict(chunks=4, straddle=160, ragged=True)),
    "full2_3x3_below_128": ("full2", 3, 3, (1, 10, 50), dict(chunks=1)),
    "full2_3x3_across_128": ("full2", 3, 3, (1, 10, 91), dict(chunks=2, straddle=128)),
    "full2_2x8_across_128": ("full2", 2, 8, (60, 89), dict(chunks=2, straddle=128)),
    "full2_2x8_across_288_ragged": ("full2", 2, 8, (1, 249), dict(chunks=4, straddle=288, ragged=True)),
    "full2_1x17_across_128": ("full2", 1, 17, (85,), dict(cross=128)),
    "full2_3x11_past_300": ("full2", 3, 11, (1, 100, 265), dict(past=300)),
    "full2_6x17_tile": ("full2", 6, 17, (1, 5, 9, 20, 40, 60), dict(tile=True)),
    "full2_8x16_cap": ("full2", 8, 16, (1, 2, 3, 5, 8, 13, 21, 34), dict(tile=False)),
    "tiny_1x1": ("tiny", 1, 1, (6,), {}),
    "tiny_2x4": ("tiny", 2, 4, (1, 20), {}),
    "tiny_3x3": ("tiny", 3, 3, (1, 10, 50), {}),
    "tiny_3x11_past_300": ("tiny", 3, 11, (1, 100, 265), dict(past=300)),
    "tiny_6x17_tile": ("tiny", 6, 17, (1, 5, 9, 20, 40, 60), dict(tile=True)),
    "tiny_6x17_tile_short": ("tiny", 6, 17, (1, 5, 9, 20, 40, 60), dict(tile=True, max_seq=128)),
    "tiny_8x16_cap": ("tiny", 8, 16, (1, 2, 3, 5, 8, 13, 21, 34), dict(tile=False)),
}
# every mode: a rows-step case, a case of 9..128 rows, the 6 x 17 case; the ragged pair in fp32, bf16_kv and bf16_act
VERIFY_BY_MODE = {
    "fp32": list(VERIFY),
    "bf16": ["full2_2x4_across_80", "full2_2x8_across_288_ragged", "full2_1x17_across_128", "full2_6x17_tile", "tiny_2x4", "tiny_6x17_tile"],
    "bf16_kv": ["full2_2x4_one_chunk", "full2_2x4_across_80", "full2_2x4_across_160_ragged", "full2_3x3_across_128",
                "full2_2x8_across_288_ragged", "full2_1x17_across_128", "full2_3x11_past_300", "full2_6x17_tile", "full2_8x16_cap",
                "tiny_1x1", "tiny_3x3", "tiny_6x17_tile", "tiny_6x17_tile_short", "tiny_8x16_cap"],
    "bf16_act": ["full2_2x4_across_80", "full2_2x4_across_160_ragged", "full2_2x8_across_128", "full2_2x8_across_288_ragged",
                 "full2_1x17_across_128", "full2_6x17_tile", "tiny_2x4", "tiny_6x17_tile"],
    "bf16_mfma": ["full2_2x4_across_80", "full2_3x3_across_128", "full2_2x8_across_288_ragged", "full2_1x17_across_128",
                  "full2_3x11_past_300", "full2_6x17_tile", "full2_8x16_cap", "tiny_2x4", "tiny_3x11_past_300", "tiny_6x17_tile",
                  "tiny_6x17_tile_short"],
}
VERIFY_CASES = [(m, c) for m in MODES for c in VERIFY_BY_MODE[m]]


def test_every_mode_sees_the_regimes_it_must():
    for mode in MODES:
        cases = [VERIFY[c] for c in VERIFY_BY_MODE[mode]]
        assert any(variant_of(m, B * T) == 5 for m, B, T, _, _ in cases), mode
        assert any(9 <= B * T <= 128 and variant_of(m, B * T) == 4 for m, B, T, _, _ in cases), mode
        assert any((B, T) == (6, 17) for _, B, T, _, _ in cases), mode
    for mode in ("fp32", "bf16_kv", "bf16_act"):
        assert any(VERIFY[c][4].get("ragged") for c in VERIFY_BY_MODE[mode]), mode


def check_regime(model, B, T, tcs, want, eng_max_seq):
    rows = B * T
    bases = [base_of(tc) for tc in tcs]
    keys = max(bases) + T                        # the keys the last row of the longest slot sees
    first = max(bases) + 1                       # ... and its first row
    print(f"  bases {bases}, rows {rows}, keys of the longest slot's rows {first}..{keys}")
    if "chunks" in want:
        assert variant_of(model, rows) == 5 and rows_step_chunks(rows, keys) == want["chunks"]
    if "straddle" in want:
        assert first <= want["straddle"] < keys
    if want.get("ragged"):
        assert min(bases) == base_of(1) and rows_step_chunks(rows, keys) == 4
    if "cross" in want:
        assert B == 1 and first <= want["cross"] < keys and variant_of(model, rows) == 4
    if "past" in want:
        assert keys > want["past"]
    if "tile" in want:
        assert (T >= 16 and B * ((T + 15) // 16) >= 12) == want["tile"]
        # with cached slots the tile attention sizes its key buffer for the context's capacity: up to 128 keys run
        # k_attention_tile_short, more run k_attention_tile (csrc/gpt_kernels.h: launch_attention_tile, nkp)
        capacity = want.get("max_seq") or ((gcfg.gpt_dims(MODELS[model])["max_seq"] + 63) // 64) * 64
        assert (((capacity + 15) & ~15) <= 128) == ("max_seq" in want)
    if "max_seq" in want:
        assert keys + 1 < eng_max_seq
    assert rows <= 128 and 2 * B <= MAX_SLOTS


@pytest.mark.parametrize("mode,case", VERIFY_CASES, ids=[f"{m}-{c}" for m, c in VERIFY_CASES])
def test_verify_matches_sequential_steps_and_the_oracle(mode, case):
    """slots 0..B-1 are prefilled one by one at their own lengths and fanned out to slots B..2B-1; the T forced tokens go through one
    gvc_gpt_verify on the first set and through T gvc_gpt_decode_step calls on the copies; one more step on both sets shows that the
    lengths and mel positions stand at base + T (a slot standing elsewhere attends to other keys at another position)."""
    model, B, T, tcs, want = VERIFY[case]
    eng, dims = engine(model, mode, want.get("max_seq"))
    L, rows = dims["n_layer"], B * T
    check_regime(model, B, T, tcs, want, want.get("max_seq", 1 << 30))
    for b, tc in enumerate(tcs):
        device_prefill(eng, model, b, 400 + b, tc)
    first, copies = torch.arange(B, device=DEV, dtype=torch.int32), torch.arange(B, 2 * B, device=DEV, dtype=torch.int32)
    eng.kv_fanout(first, copies)
    gen = torch.Generator().manual_seed(1000 + 17 * B + T)
    toks = torch.randint(0, 1024, (B, T), generator=gen).to(torch.int32)
    nxt = torch.randint(0, 1024, (B,), generator=gen).to(torch.int32)
    b16_0, rows_0 = eng.bf16_gemm_launches(), eng.rows_step_launches()
    vl, vz = eng.verify(first, toks.to(DEV))
    variant = eng.decode_variant()
    b16_v, rows_v = eng.bf16_gemm_launches() - b16_0, eng.rows_step_launches() - rows_0
    seq = [eng.decode_step(copies, toks[:, t].contiguous().to(DEV)) for t in range(T)]
    sl_, sz = torch.stack([a for a, _ in seq], 1), torch.stack([b for _, b in seq], 1)
    al, az = eng.decode_step(first, nxt.to(DEV))
    bl, bz = eng.decode_step(copies, nxt.to(DEV))
    torch.cuda.synchronize()
    eng.health()
    act_v, act_s = act_rows(model, mode, rows), act_rows(model, mode, B)
    print(f"{mode} {case}: decode variant {variant}, bf16 strip GEMMs {b16_v}, rows-step launches {rows_v}, activations rounded in the "
          f"pass: {act_v}, in the sequential steps: {act_s}")
    assert variant == variant_of(model, rows)
    assert (rows_v > 0) == (variant == 5)
    # the bf16 strip path: four matrix-core GEMMs per layer for every pass of 2+ rows of a bf16_mfma context that is not a rows step
    assert b16_v == (4 * L if mode == "bf16_mfma" and variant == 4 and rows > 1 else 0)
    vs_oracle, vs_seq, seq_vs_oracle = Check("pass vs oracle", mode), Check("pass vs sequential steps", mode), None
    if act_v != act_s:
        seq_vs_oracle = Check("sequential steps vs oracle with their rounding points", mode)
    for b, tc in enumerate(tcs):
        o = Twin(model, mode, 400 + b, tc)
        os_ = o.fork()
        ol, oz, ball = o.rows(toks[b], act_v)
        nl, nz, nball = o.rows(nxt[b:b + 1], act_s)
        vs_oracle.add(vl[b], vz[b], ol, oz, ball)
        vs_oracle.add(al[b:b + 1], az[b:b + 1], nl, nz, nball)
        if seq_vs_oracle is None:
            vs_seq.add(vl[b], vz[b], sl_[b], sz[b], ball)
            vs_seq.add(al[b:b + 1], az[b:b + 1], bl[b:b + 1], bz[b:b + 1], nball)
        else:
            outs = [os_.rows(toks[b, t:t + 1], act_s) for t in range(T)]
            ol2, oz2 = torch.cat([x[0] for x in outs]), torch.cat([x[1] for x in outs])
            ball2 = torch.cat([x[2] for x in outs]) if outs[0][2] is not None else None
            nl2, nz2, nball2 = os_.rows(nxt[b:b + 1], act_s)
            seq_vs_oracle.add(sl_[b], sz[b], ol2, oz2, ball2)
            seq_vs_oracle.add(bl[b:b + 1], bz[b:b + 1], nl2, nz2, nball2)
    vs_oracle.finish()
    (seq_vs_oracle or vs_seq).finish()


@pytest.mark.parametrize("model", ["tiny", "full2"])
@pytest.mark.parametrize("mode", MODES)
def test_verify_rollback_verify_loop(mode, model):
    """The loop speculative decoding runs: verify 7, truncate [3, 0], verify 5 other tokens (which overwrite the stale rows), truncate
    [5, 1] (a whole round dropped on slot 0), one decode step.  The mirror slots never roll back: they are fanned-out copies of the
    same contexts driven with one two-row decode step per token and are handed the KEPT tokens only -- a mirror for a shorter history is
    a snapshot (kv_fanout, an exact copy: section 2) taken while the longer one was stepped.  Both passes and the last step against the
    mirror and against the oracle."""
    eng, dims = engine(model, mode)
    tcs, T1, T2 = (6, 30), 7, 5
    for b, tc in enumerate(tcs):
        device_prefill(eng, model, b, 420 + b, tc)
    eng.kv_fanout(sl(0, 1), sl(2, 3))
    gen = torch.Generator().manual_seed(77)
    t1 = torch.randint(0, 1024, (2, T1), generator=gen).to(torch.int32)
    t2 = torch.randint(0, 1024, (2, T2), generator=gen).to(torch.int32)
    nxt = torch.randint(0, 1024, (2,), generator=gen).to(torch.int32)
    step = lambda slots, col: eng.decode_step(slots, col.contiguous().to(DEV))
    # round 1: slot 0 keeps 4 of its 7 tokens, slot 1 all 7
    v1 = eng.verify(sl(0, 1), t1.to(DEV))
    variant = eng.decode_variant()
    m1 = []
    for t in range(T1):
        if t == T1 - 3:
            eng.kv_fanout(sl(2), sl(4))                       # slot 4: slot 0's history after the rollback
        m1.append(step(sl(2, 3), t1[:, t]))
    eng.kv_fanout(sl(3), sl(5))                               # slot 5: slot 1's (nothing dropped)
    eng.truncate(sl(0, 1), sl(3, 0))
    # round 2 behind the kept tokens: slot 0 then drops all 5, slot 1 the last one
    eng.kv_fanout(sl(4), sl(6))                               # slot 6: slot 0's history after the second rollback
    v2 = eng.verify(sl(0, 1), t2.to(DEV))
    m2 = []
    for t in range(T2):
        if t == T2 - 1:
            eng.kv_fanout(sl(5), sl(7))                       # slot 7: slot 1's history after the second rollback
        m2.append(step(sl(4, 5), t2[:, t]))
    eng.truncate(sl(0, 1), sl(5, 1))
    a = step(sl(0, 1), nxt)
    m = step(sl(6, 7), nxt)
    torch.cuda.synchronize()
    eng.health()
    assert variant == variant_of(model, 2 * T1)
    act_v1, act_v2, act_s = act_rows(model, mode, 2 * T1), act_rows(model, mode, 2 * T2), act_rows(model, mode, 2)
    assert act_v1 == act_v2 == act_s, "the passes and the two-row mirror steps round at the same points in every mode"
    print(f"{mode} {model}: decode variant {variant}, activations rounded: {act_s}")
    stack = lambda seq, i: torch.stack([x[i] for x in seq], 1)
    vs_mirror, vs_oracle = Check("passes and last step vs mirror", mode), Check("passes and last step vs oracle", mode)
    for b, tc in enumerate(tcs):
        o = Twin(model, mode, 420 + b, tc)
        l1, z1, ball1 = o.rows(t1[b], act_v1)
        o.drop((3, 0)[b])
        l2, z2, ball2 = o.rows(t2[b], act_v2)
        o.drop((5, 1)[b])
        l3, z3, ball3 = o.rows(nxt[b:b + 1], act_s)
        assert CO.cache_len(o.caches[0]) == base_of(tc) + (T1 - 3 + 1, T1 + T2 - 1 + 1)[b]
        for got, mir, ref in (((v1[0][b], v1[1][b]), (stack(m1, 0)[b], stack(m1, 1)[b]), (l1, z1, ball1)),
                              ((v2[0][b], v2[1][b]), (stack(m2, 0)[b], stack(m2, 1)[b]), (l2, z2, ball2)),
                              ((a[0][b:b + 1], a[1][b:b + 1]), (m[0][b:b + 1], m[1][b:b + 1]), (l3, z3, ball3))):
            vs_mirror.add(got[0], got[1], mir[0], mir[1], ref[2])
            vs_oracle.add(got[0], got[1], ref[0], ref[1], ref[2])
    vs_mirror.finish()
    vs_oracle.finish()


# ---- 2. KV fan-out ------------------------------------------------------------------------------------------------------------------
# fp32 and bf16_kv on all three head sizes (64, 128, 256: a cache row of 128 * 2 bytes at d 512); bf16_act and bf16_mfma share
# bf16_kv's cache layout: one model each
FANOUT_CASES = [(m, mode) for mode in ("fp32", "bf16_kv") for m in ("tiny", "d512", "full2")] + [("full2", "bf16_act"), ("tiny", "bf16_mfma")]


def _rows_equal(out, what):
    logits, latent = out
    for r in range(1, logits.shape[0]):
        assert torch.equal(logits[r], logits[0]) and torch.equal(latent[r], latent[0]), f"{what}: row {r} differs from row 0"


@pytest.mark.parametrize("model,mode", FANOUT_CASES, ids=[f"{mode}-{m}" for m, mode in FANOUT_CASES])
def test_kv_fanout_copies_are_exact(model, mode):
    """The copy is a byte copy and the rows of one decode step are computed alike, so source and copies, fed the same token as rows of
    ONE call, answer bit for bit: 1 -> 1, 1 -> 7, and a list with a src == dst pair and out-of-range slots, which copy nothing (slot 9,
    named as the destination of two out-of-range sources, still equals slot 8, which was prefilled like it)."""
    eng, dims = engine(model, mode)
    device_prefill(eng, model, 0, 440, 9)
    device_prefill(eng, model, 8, 441, 4)
    device_prefill(eng, model, 9, 441, 4)
    for t in (3, 900, 77):
        eng.decode_step(sl(0), sl(t))
    tok = lambda n, t: torch.full((n,), t, device=DEV, dtype=torch.int32)
    eng.kv_fanout(sl(0), sl(1))
    _rows_equal(eng.decode_step(sl(0, 1), tok(2, 5)), "1 -> 1")
    eng.kv_fanout(sl(0, 0, 0, 0, 0, 0, 0), sl(1, 2, 3, 4, 5, 6, 7))
    _rows_equal(eng.decode_step(torch.arange(8, device=DEV, dtype=torch.int32), tok(8, 6)), "1 -> 7")
    eng.kv_fanout(sl(0, 0, 8, MAX_SLOTS, -1), sl(10, 0, 99, 9, 9))
    _rows_equal(eng.decode_step(sl(0, 1, 2, 3, 4, 5, 6, 7, 10), tok(9, 7)), "list: 0 -> 10")
    _rows_equal(eng.decode_step(sl(8, 9), tok(2, 8)), "list: slot 9 untouched")
    # against the oracle, so that "all rows equal" is not "all rows equally wrong": one more step of two copies, which have taken
    # the source's three one-row steps and then tokens 5, 6, 7 in steps of 2, 8 and 9 rows
    got = eng.decode_step(sl(10, 3), tok(2, 8))
    torch.cuda.synchronize()
    eng.health()
    o = Twin(model, mode, 440, 9)
    for t, n in ((3, 1), (900, 1), (77, 1), (5, 2), (6, 8), (7, 9)):
        o.rows(torch.tensor([t]), act_rows(model, mode, n))
    ol, oz, ball = o.rows(torch.tensor([8]), act_rows(model, mode, 2))
    c = Check(f"{mode} {model}: a copy's step vs oracle", mode)
    for r in range(2):
        c.add(got[0][r:r + 1], got[1][r:r + 1], ol, oz, ball)
    c.finish()


@pytest.mark.parametrize("model,mode", [("full2", "fp32"), ("full2", "bf16_kv"), ("d512", "bf16_kv")])
def test_kv_fanout_takes_a_deferred_token_and_the_parked_rows_along(model, mode):
    """A plain one-stream generate on the one-launch step leaves its last token pending in the slot and the next step's logits / latent
    parked beside it.  A fan-out of that slot takes all three along: the generation continued from the copy (cloned loop buffers) emits
    the source's tokens and latents, and the next eager step from both agrees bit for bit -- and with a slot that was fed the emitted
    tokens eagerly, to the mode's tolerance."""
    from genvc_amd.engine import sample_params
    eng, dims = engine(model, mode)
    cond, codes = slot_inputs(model, 450, 9)
    prefix = eng.prefix_embeddings(cond.to(DEV), codes.to(DEV).int())
    P, n, d = prefix.shape[1], 12, dims["d_model"]
    sp = sample_params(dict(gcfg.DEFAULT_SAMPLING, top_k=1), V, EOS)
    buf = dict(ids=torch.ones(1, P + 1 + n + 8, device=DEV, dtype=torch.int32), ids_len=torch.full((1,), P + 1, device=DEV, dtype=torch.int32),
               fin=torch.zeros(1, device=DEV, dtype=torch.int32), toks=torch.full((1, n), -1, device=DEV, dtype=torch.int32),
               lats=torch.zeros(1, n, d, device=DEV))
    buf["ids"][:, P] = dims["start_audio_token"]
    gen = lambda slot, b, i0, k: eng.generate(sl(slot), b["ids"], b["ids_len"], b["fin"], sp, i0, k, b["toks"], b["lats"], max_keys=P + 1 + n)
    eng.prefill(sl(0), prefix, want_outputs=False)
    eng.prefill(sl(2), prefix, want_outputs=False)
    gen(0, buf, 0, 5)
    assert eng.decode_variant() == 3, "not on the one-launch step: nothing was deferred"
    eng.kv_fanout(sl(0), sl(1))
    twin = {k: v.clone() for k, v in buf.items()}
    gen(0, buf, 5, 4)
    gen(1, twin, 5, 4)
    torch.cuda.synchronize()
    assert not bool(buf["fin"].any()), "the stream stopped: choose another input seed"
    for k in buf:
        assert torch.equal(buf[k], twin[k]), f"{k} differs between the source's and the copy's continuation"
    probe = sl(11)
    a, b = eng.decode_step(sl(0), probe), eng.decode_step(sl(1), probe)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for t in buf["toks"][0, :9]:
        eng.decode_step(sl(2), t.view(1).contiguous())
    e = eng.decode_step(sl(2), probe)
    torch.cuda.synchronize()
    eng.health()
    c = Check(f"{mode} {model}: the copy's next step vs an eagerly fed slot", mode)
    c.add(b[0], b[1], e[0], e[1])
    c.finish()


# ---- 3. beam span copies in the bf16-cache modes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("model,B,K,steps", [("tiny", 2, 4, 11), ("full2", 2, 4, 11), ("full2", 1, 3, 17)])
@pytest.mark.parametrize("mode", ["bf16_kv", "bf16_mfma"])
def test_beam_slots_hold_the_kv_a_replay_writes_bf16_cache(mode, model, B, K, steps):
    """test_gpu_beam.test_beam_slots_hold_the_kv_a_replay_writes with a bf16 cache (the span copies and the step-0 fan-out move
    2-byte elements): after beam_generate every beam slot answers a probe step like a spare slot into which its own token history was
    replayed, and like the oracle.  The replay runs two rows at a time, so that it rounds where the beam's B * K-row steps round (a
    bf16_mfma context rounds activations in every pass of 2+ rows, not in a one-row step); the probe goes to fanned-out copies of the
    beam slots (exact copies: section 2), which leaves the beams as they are and lets pairs overlap when B * K is odd.  At d = 1024
    the B * K rows take the one-launch rows step."""
    from genvc_amd.engine import BeamSearch
    eng, dims = engine(model, mode)
    BK = B * K
    cond, codes = slot_inputs(model, 2950, 9, B)
    prefix = eng.prefix_embeddings(cond.to(DEV), codes.to(DEV).int())
    fake = torch.ones(B, prefix.shape[1] + 1, dtype=torch.long, device=DEV)
    fake[:, -1] = dims["start_audio_token"]
    n0 = int(fake.shape[1])
    slots = torch.arange(BK, device=DEV, dtype=torch.int32)
    eng.prefill(slots[::K].contiguous(), prefix, want_outputs=False)
    beam = BeamSearch(fake, K, 40, EOS, V, 1.0, 2.0, "4.33")
    eng.beam_generate(slots, beam, 1)                      # step 0: every child has parent 0 -- K-1 copies of one slot
    assert int(beam.n_copies[0]) == K - 1
    eng.beam_generate(slots, beam, steps - 1)
    torch.cuda.synchronize()
    eng.health()
    if model == "full2":
        assert eng.decode_variant() == 5, "the beams' steps did not run on the one-launch rows step"
    T = beam.steps
    toks = beam.ids[T & 1, :, n0:n0 + T].clone()
    spare, probed = sl(BK, BK + 1), sl(BK + 2, BK + 3)
    probe = sl(7, 7)
    act = act_rows(model, mode, BK)
    assert act == act_rows(model, mode, 2)
    vs_replay, vs_oracle = Check("beam slots vs replay", mode), Check("beam slots vs oracle", mode)
    odims = oracle_setup(model, mode)[1]
    runs = [(oracle_setup(model, mode, dbl)[0], cond.double() if dbl else cond) for dbl in ([False, True] if mode in ACT_MODES else [False])]
    for r in sorted(set(list(range(0, BK - 1, 2)) + [BK - 2])):
        pair = [r, r + 1]
        items = [p // K for p in pair]
        eng.reset(spare)
        eng.prefill(spare, prefix[items].contiguous(), want_outputs=False)
        for j in range(T):
            eng.decode_step(spare, toks[pair, j].contiguous())
        ref = eng.decode_step(spare, probe)
        eng.kv_fanout(slots[pair].contiguous(), probed)
        got = eng.decode_step(probed, probe)
        for i, p in enumerate(pair):
            outs = []
            for w, cnd in runs:
                c = CO.prefill(w, odims, cnd[items[i]:items[i] + 1], codes[items[i]:items[i] + 1], act=mode == "bf16_mfma")[2]
                _, _, c = CO.forced_rows(w, odims, c, toks[p].cpu(), 1, act=act)
                outs.append(CO.forced_rows(w, odims, c, torch.tensor([7]), 1 + T, act=act))
            ball = (outs[1][1].float() - outs[0][1]).abs() if len(outs) > 1 else None
            vs_replay.add(got[0][i:i + 1], got[1][i:i + 1], ref[0][i:i + 1], ref[1][i:i + 1], ball)
            vs_oracle.add(got[0][i:i + 1], got[1][i:i + 1], outs[0][0], outs[0][1], ball)
    torch.cuda.synchronize()
    eng.health()
    print(f"{mode} {model} B {B} K {K} steps {steps}:")
    vs_replay.finish()
    vs_oracle.finish()


# ---- 4. cached-prefix prefill with a bf16 cache --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tn", [(1, 15), (1, 16), (6, 17)])
@pytest.mark.parametrize("model", ["tiny", "full2"])
def test_cached_prefix_prefill_bf16_kv(model, B, Tn):
    """prefill(..., n_cached=32) of a second segment (Tn = Tc + 3 uncached rows per slot) onto the conditioning rows a first segment
    left in a bf16 cache: 15 and 16 rows of one slot (either side of the tile attention's T >= 16; at d = 1024 both on the one-launch
    rows step with its 16-row instantiation) and 6 x 17 rows (the tile attention under base_len, reading bf16 keys).  The last row of
    the cached prefill against the same row of one uncached prefill of the whole sequence on fresh slots and against the oracle, then
    one decode step behind both."""
    mode = "bf16_kv"
    eng, dims = engine(model, mode)
    w, odims = oracle_setup(model, mode)
    cond, codes_a = slot_inputs(model, 460, 9, B)
    codes_b = synth.integers(461, "content_codes", (B, Tn - 3), 256)
    cached = torch.arange(B, device=DEV, dtype=torch.int32)
    fresh = cached + 8
    eng.prefill(cached, eng.prefix_embeddings(cond.to(DEV), codes_a.to(DEV).int()), want_outputs=False)
    eng.decode_step(cached, torch.full((B,), 5, device=DEV, dtype=torch.int32))              # ... and decodes a little
    pb = eng.prefix_embeddings(cond.to(DEV), codes_b.to(DEV).int())
    assert pb.shape[1] + 1 - 32 == Tn
    rows_0 = eng.rows_step_launches()
    lg_c, lat_c = eng.prefill(cached, pb, n_cached=32)
    rows_c = eng.rows_step_launches() - rows_0
    lg_f, lat_f = eng.prefill(fresh, pb)
    tok = torch.randint(0, 1024, (B,), generator=torch.Generator().manual_seed(Tn)).to(torch.int32)
    a, f = eng.decode_step(cached, tok.to(DEV)), eng.decode_step(fresh, tok.to(DEV))
    torch.cuda.synchronize()
    eng.health()
    print(f"{model} {B} x {Tn} uncached rows: rows-step launches of the cached prefill {rows_c}")
    assert (rows_c > 0) == (model == "full2" and B * Tn <= 16)
    z, logits, cache = CO.prefill(w, odims, cond, codes_b)
    vs_full, vs_oracle = Check("cached vs uncached prefill", mode), Check("cached prefill vs oracle", mode)
    vs_full.add(lg_c, lat_c, lg_f, lat_f)
    vs_full.add(a[0], a[1], f[0], f[1])
    vs_oracle.add(lg_c, lat_c, logits, z)
    for b in range(B):
        cb = [(k[b:b + 1], v[b:b + 1]) for k, v in cache]
        nl, nz, _ = CO.forced_rows(w, odims, cb, tok[b:b + 1], 1)
        vs_oracle.add(a[0][b:b + 1], a[1][b:b + 1], nl, nz)
    vs_full.finish()
    vs_oracle.finish()
