"""GPU: weight_dtype 4 ("bf16_mfma", include/genvc_hip.h) -- every multi-row pass of the GPT that is not a one-launch step runs its four
projections per layer on bf16 matrix cores (csrc/gemm_b16.hip) with the rounding points of the one-launch bf16 rows step, against the
oracle with the same rounding points (`gpt_blocks(act_bf16, kv_bf16)`, `gpt_prefill(act_bf16_prefill)`; reference block math
layers/gpt_inference.py:81-112, loop layers/stream_generator.py:809-881).

bf16 rounding makes the map discontinuous, so the yardstick is the one of test_gpu_round6.test_rows_step_bf16_activations_vs_oracle: the
oracle re-run on a conditioning input perturbed by 2e-7 relative; the HIP path must stay within 3x of that (median + 1e-4, 99.9 %
quantile + 1e-3)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from genvc_amd import config as gcfg
from genvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GREEDY = dict(gcfg.DEFAULT_SAMPLING, top_k=1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE2 = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2, gpt_n_heads=4)
ACT = dict(kv_bf16=True, act_bf16=True, act_bf16_prefill=True)

_weights = {}


def _q(t, p):
    return float(torch.quantile(t.flatten()[::max(1, t.numel() // 200000)].double(), p))


def _setup(margs):
    """(dims, device weights, bf16-rounded CPU weights) of make_weights(5, ...), built once per model shape"""
    from test_gpu_gpt import _round_bf16
    key = tuple(sorted(margs.items()))
    if key not in _weights:
        dims = gcfg.gpt_dims(margs)
        w = synth.make_weights(5, synth.gpt_weight_spec(dims), device=DEV)
        _weights[key] = (dims, w, _round_bf16({k: v.cpu() for k, v in w.items()}))
    return _weights[key]


def _engine(dims, w, mode, max_slots=8):
    from genvc_amd.engine import GptEngine
    torch.cuda.empty_cache()
    eng = GptEngine(dims, max_slots=max_slots, max_rows=2048, weight_dtype=mode)
    eng.bind(w)
    return eng


def _rows(O, wr, dims, cond, codes):
    """the prefill's input rows [prefix | mel_embedding[start] + mel_pos[0]] as gpt_prefill builds them"""
    prefix = O.compute_embeddings(wr, dims, cond, codes)[0]
    row = wr["mel_embedding.weight"][dims["start_audio_token"]] + wr["mel_pos_embedding.emb.weight"][0]
    return prefix, torch.cat([prefix, row.view(1, 1, -1).expand(prefix.shape[0], 1, -1)], dim=1)


def _perturbed(cond):
    g = torch.Generator().manual_seed(0)
    return cond * (1 + 2e-7 * torch.randn(cond.shape, generator=g))


def _within_yardstick(d_hip, d_ref, what):
    print(f"{what}: median {_q(d_hip, 0.5):.3e} (yardstick {_q(d_ref, 0.5):.3e}), 99.9 % {_q(d_hip, 0.999):.3e} (yardstick {_q(d_ref, 0.999):.3e})")
    assert _q(d_hip, 0.5) <= 3.0 * _q(d_ref, 0.5) + 1e-4, (what, _q(d_hip, 0.5), _q(d_ref, 0.5))
    assert _q(d_hip, 0.999) <= 3.0 * _q(d_ref, 0.999) + 1e-3, (what, _q(d_hip, 0.999), _q(d_ref, 0.999))


TINY1 = dict(gcfg.TINY_MODEL_ARGS, gpt_layers=1)


@pytest.mark.parametrize("margs,B,Tc,in_seed,sharp", [
    (TINY1, 2, 13, 100, True), (TINY1, 3, 75, 103, True), (gcfg.TINY_MODEL_ARGS, 3, 75, 100, False), (WIDE2, 8, 13, 100, False),
    (dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2, gpt_n_heads=16), 1, 20, 101, False)],
    ids=["tiny_1_layer_96_rows", "tiny_1_layer_330_rows", "tiny_330_rows", "d1024_384_rows_head_dim_256", "d1024_55_rows_head_dim_64"])
def test_prefill_hidden_vs_oracle_with_the_same_rounding_points(margs, B, Tc, in_seed, sharp):
    """ln_f of every prefill row against `gpt_blocks(act_bf16=True, kv_bf16=True)`.  The two one-layer tiny cases are the sharp ones: there
    the median bar is ~1e-4 and the oracle WITHOUT activation rounding (mode-2 arithmetic) misses it, which is asserted -- a wiring
    that silently computes as mode 2 cannot pass.  At d = 1024 the bar does not separate the two arithmetics (measured): those cases
    check layout, head shapes and row counts.  The bf16 GEMM counter advances by four launches per layer."""
    from oracle import genvc_oracle as O
    dims, w, wr = _setup(margs)
    d = dims["d_model"]
    dims_o = dict(dims, kv_bf16=True, act_bf16=True)
    cond = synth.uniform(in_seed, "cond_latents", (B, 32, d), 1.0)
    codes = synth.integers(in_seed, "content_codes", (B, Tc), 256)
    prefix, emb = _rows(O, wr, dims, cond, codes)
    ref = O.gpt_blocks(wr, dims_o, emb)[0]
    pert = O.gpt_blocks(wr, dims_o, _rows(O, wr, dims, _perturbed(cond), codes)[1])[0]
    d_ref = (pert - ref).abs()
    if sharp:
        d_m2 = (O.gpt_blocks(wr, dict(dims, kv_bf16=True), emb)[0] - ref).abs()
        assert _q(d_m2, 0.5) > 3.0 * _q(d_ref, 0.5) + 1e-4, "the bar no longer tells mode-2 arithmetic from the mode's rounding points"
    eng = _engine(dims, w, "bf16_mfma")
    hidden = torch.full((B, prefix.shape[1] + 1, d), float("nan"), device=DEV)
    before = eng.bf16_gemm_launches()
    eng.prefill_hidden(torch.arange(B, device=DEV, dtype=torch.int32), prefix.to(DEV), hidden)
    torch.cuda.synchronize()
    assert eng.bf16_gemm_launches() - before == 4 * dims["n_layer"]
    eng.health()
    eng.close()
    _within_yardstick((hidden.cpu() - ref).abs(), d_ref, f"prefill_hidden {B} x {prefix.shape[1] + 1} rows, d {d}")


@pytest.mark.parametrize("mode", ["fp32", "bf16_kv", "bf16_act"])
def test_other_modes_never_launch_the_bf16_gemms(mode):
    """a context of mode 0, 2 or 3 keeps its launch sequence: the counter stays 0 across a prefill_hidden, a prefill and 8 decode steps"""
    from test_gpu_gpt import run_generate
    dims, w, _ = _setup(WIDE2)
    eng = _engine(dims, w, mode)
    cond = synth.uniform(100, "cond_latents", (8, 32, 1024), 1.0)
    codes = synth.integers(100, "content_codes", (8, 13), 256)
    prefix = eng.prefix_embeddings(cond.to(DEV), codes.to(DEV).int())
    eng.prefill_hidden(torch.arange(8, device=DEV, dtype=torch.int32), prefix, torch.empty(8, prefix.shape[1] + 1, 1024, device=DEV))
    run_generate(eng, dims, cond, codes, 8)
    torch.cuda.synchronize()
    assert eng.bf16_gemm_launches() == 0
    eng.close()


_gen_ref = {}


def _generation_reference():
    """the oracle's greedy run of the 8-stream case, its perturbed re-run (teacher-forced on the first run's tokens) and its margins"""
    if not _gen_ref:
        from oracle import genvc_oracle as O
        from test_gpu_round6 import _greedy_margins
        dims, w, wr = _setup(WIDE2)
        dims_o = dict(dims, **ACT)
        B, Tc, n = 8, 13, 16
        cond = synth.uniform(100, "cond_latents", (B, 32, 1024), 1.0)
        codes = synth.integers(100, "content_codes", (B, Tc), 256)
        ref_t, ref_l, ref_logits = O.generate(wr, dims_o, cond, codes, GREEDY, max_new=n, stop_on_eos=False)
        prefix, _ = O.compute_embeddings(wr, dims_o, _perturbed(cond), codes)
        z, _, cache = O.gpt_prefill(wr, dims_o, prefix)
        pert = [z]
        for j in range(1, n):
            z, _, cache = O.gpt_decode_step(wr, dims_o, cache, ref_t[:, j - 1], j)
            pert.append(z)
        _gen_ref.update(cond=cond, codes=codes, n=n, ref_t=ref_t, ref_l=ref_l, pert_l=torch.stack(pert, 1),
                        margins=_greedy_margins(O, ref_t, ref_logits, B, Tc, n))
    return _gen_ref


def _check_generation(toks, lats, what):
    """the assertions of test_rows_step_bf16_activations_vs_oracle, with step 0 (the prefill's row) held to the same yardstick"""
    R = _generation_reference()
    ref_t, ref_l, pert_l, margins, n = R["ref_t"], R["ref_l"], R["pert_l"], R["margins"], R["n"]
    B = ref_t.shape[0]
    agree = toks == ref_t
    first = min(int((~agree[b]).nonzero()[0]) if (~agree[b]).any() else n for b in range(B))
    assert first >= 2
    _within_yardstick((lats[:, :first] - ref_l[:, :first]).abs(), (pert_l[:, :first] - ref_l[:, :first]).abs(), what)
    assert float(agree.float().mean()) >= 0.85, float(agree.float().mean())
    for b in range(B):
        bad = (~agree[b]).nonzero()
        if len(bad):
            assert float(margins[b, int(bad[0])]) < 2e-2, (b, int(bad[0]), float(margins[b, int(bad[0])]))


def test_greedy_generation_8_streams_vs_oracle():
    """prefill on the bf16 GEMM path, 16 greedy steps on the one-launch bf16 rows step (decode variant 5), against the oracle with
    activation rounding in the prefill too"""
    from test_gpu_gpt import run_generate
    R = _generation_reference()
    dims, w, _ = _setup(WIDE2)
    eng = _engine(dims, w, "bf16_mfma")
    before = eng.bf16_gemm_launches()
    _, toks, lats = run_generate(eng, dims, R["cond"], R["codes"], R["n"])
    assert eng.decode_variant() == 5, "the decode steps did not run on the one-launch rows step"
    assert eng.bf16_gemm_launches() - before == 4 * dims["n_layer"], "the prefill alone runs on the bf16 GEMMs here"
    torch.cuda.synchronize()
    eng.health()
    eng.close()
    _check_generation(toks.long(), lats, "8 streams, rows step")


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[2])
from genvc_amd import config as gcfg, synth
from genvc_amd.engine import GptEngine
from test_gpu_gpt import run_generate
dims = gcfg.gpt_dims(dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2, gpt_n_heads=4))
w = synth.make_weights(5, synth.gpt_weight_spec(dims), device="cuda")
eng = GptEngine(dims, max_slots=8, max_rows=2048, weight_dtype="bf16_mfma")
eng.bind(w)
cond = synth.uniform(100, "cond_latents", (8, 32, 1024), 1.0)
codes = synth.integers(100, "content_codes", (8, 13), 256)
_, toks, lats = run_generate(eng, dims, cond, codes, 16)
torch.cuda.synchronize()
eng.health()
after_loop = eng.bf16_gemm_launches()
slots = torch.arange(8, device="cuda", dtype=torch.int32)
per_step = []
for _ in range(2):
    c0 = eng.bf16_gemm_launches()
    eng.decode_step(slots, torch.full((8,), 5, device="cuda", dtype=torch.int32))
    per_step.append(eng.bf16_gemm_launches() - c0)
torch.cuda.synchronize()
eng.health()
np.savez(sys.argv[1], toks=toks.numpy(), lats=lats.numpy(), after_loop=after_loop, per_step=np.array(per_step),
         rows_steps=eng.rows_step_launches(), layers=dims["n_layer"])
eng.close()
"""


def test_rows_step_switched_off_keeps_the_rounding_points(tmp_path):
    """GVC_PERSIST_ROWS=0 (the documented switch; what a hand-off time-out leaves behind as well): the 8-row decode steps of the same case
    run on the bf16 GEMM path -- no one-launch rows step, four bf16 GEMMs per layer and eager step -- and the latents meet the same
    bars.  A fresh child process, because the switch is read when the context is created."""
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, GVC_PERSIST_ROWS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, out, os.path.join(ROOT, "tests")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    L = int(z["layers"])
    assert int(z["rows_steps"]) == 0, "the one-launch rows step ran although it was switched off"
    assert int(z["after_loop"]) > 4 * L, "the decode steps of the loop did not reach the bf16 GEMMs"
    assert list(z["per_step"]) == [4 * L, 4 * L], "an eager 8-row decode step is four bf16 GEMMs per layer"
    _check_generation(torch.from_numpy(z["toks"]).long(), torch.from_numpy(z["lats"]), "8 streams, rows step off")


def test_cached_chunk_prefill_8x16_rows_vs_oracle():
    """the streams leg's shape: 8 streams x 16 uncached rows (text rows + start token) behind 32 cached conditioning rows left by a 48-row
    prefill -- 128 rows, past the one-launch rows step, on the bf16 GEMM path with positions base_len + t.  The chunk's last-row latents
    against the oracle continuing its own cache (the conditioning rows' k / v of its first pass)."""
    from oracle import genvc_oracle as O
    dims, w, wr = _setup(WIDE2)
    dims_o = dict(dims, kv_bf16=True, act_bf16=True)
    B = 8
    cond = synth.uniform(100, "cond_latents", (B, 32, 1024), 1.0)
    codes_a = synth.integers(100, "content_codes", (B, 13), 256)
    codes_b = synth.integers(101, "content_codes", (B, 13), 256)

    def oracle(cnd):
        _, cache = O.gpt_blocks(wr, dims_o, _rows(O, wr, dims, cnd, codes_a)[1])
        cache = [(k[:, :, :32], v[:, :, :32]) for k, v in cache]
        h, _ = O.gpt_blocks(wr, dims_o, _rows(O, wr, dims, cnd, codes_b)[1][:, 32:], cache)
        return O.head(wr, h[:, -1])[0]

    ref, pert = oracle(cond), oracle(_perturbed(cond))
    eng = _engine(dims, w, "bf16_mfma")
    slots = torch.arange(B, device=DEV, dtype=torch.int32)
    eng.prefill(slots, _rows(O, wr, dims, cond, codes_a)[0].to(DEV), want_outputs=False)
    before, rows_before = eng.bf16_gemm_launches(), eng.rows_step_launches()
    _, lat = eng.prefill(slots, _rows(O, wr, dims, cond, codes_b)[0].to(DEV), n_cached=32)
    torch.cuda.synchronize()
    assert eng.bf16_gemm_launches() - before == 4 * dims["n_layer"] and eng.rows_step_launches() == rows_before
    eng.health()
    eng.close()
    _within_yardstick((lat.cpu() - ref).abs(), (pert - ref).abs(), "cached chunk prefill 8 x 16 rows")
