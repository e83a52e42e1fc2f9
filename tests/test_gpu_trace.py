"""GPU: attentions and hidden states of GPT.generate (output_attentions / output_hidden_states), GPT.trace and the content alignment
(include/genvc_hip.h: gvc_gpt_trace; csrc/trace.h: k_attention_probs) against tests/golden/trace_*.npz -- the reference's
GPT2InferenceModel driven step by step with eager attention (scripts/make_trace_golden.py) -- and against tests/trace_oracle.py where
a fixture cannot reach (the device's own sampled ids, other weight presets).

Tolerances: 8 x floor, the floor being the reference's own fp32-versus-fp64 deviation max(max|fp32 - fp64|, 2^-24 max|value|), stored
by the fixture script or computed by the oracle on the ids at hand.  Every comparison prints its figure first."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import act_stats                              # noqa: E402
import trace_oracle as TO                     # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 8.0                  # floors
N_COND = TO.N_COND
ASK = dict(return_dict_in_generate=True, output_attentions=True, output_hidden_states=True)

_gpt, _w = {}, {}


def weights(tag, seed, stop_bias=None, preset=TO.PEAKED):
    key = (tag, seed, stop_bias, repr(preset))
    if key not in _w:
        _w[key] = TO.case_weights(tag, seed, stop_bias, preset)
    return _w[key]


def make_gpt(tag, w, key=None, weight_dtype="fp32", max_slots=8):
    """a GPT of the case's dims on the device with weights w, built once per session under `key`"""
    if key is not None and key in _gpt:
        return _gpt[key]
    from genvc_amd.layers.gpt import GPT
    a = TO.CASES[tag]
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    g.load_state_dict(w, strict=False)
    g.to(DEV)
    g.init_gpt_for_inference(max_slots=max_slots, weight_dtype=weight_dtype)
    if key is not None:
        _gpt[key] = g
    return g


def fixture_gpt(tag, gold):
    f = gold(f"trace_{tag}")
    seed, bias = int(f["seed"]), float(f["stop_bias"])
    bias = None if bias < 0 else bias
    return f, make_gpt(tag, weights(tag, seed, bias), key=("fixture", tag)), TO.case_inputs(tag, seed)


def floors(w, dims, cond, codes, ids, lengths):
    """(probs32, hidden32, floor_att, floor_hid) of the oracle on these ids: its fp32 run against its fp64 run"""
    p32, h32 = TO.trace(w, dims, cond, codes, ids, lengths)
    p64, h64 = TO.trace(act_stats.double(w), dims, cond.double(), codes, ids, lengths)
    fl = lambda a, b: max(float((a.double() - b).abs().max()), 2.0 ** -24 * float(b.abs().max()))
    return p32, h32, p64, h64, fl(p32, p64), fl(h32, h64)


def stack_steps(steps, full_shape, P):
    """HF's per-step views put back into a full [L, rows, ..., T, ...] tensor on the CPU (zeros elsewhere): attentions or hidden states"""
    out = torch.zeros(full_shape)
    for i, layers in enumerate(steps):
        lo = 0 if i == 0 else P + i
        for l, v in enumerate(layers):
            if out.ndim == 5:
                out[l][:, :, lo:P + i + 1, :P + i + 1] = v.cpu()
            else:
                out[l][:, lo:P + i + 1] = v.cpu()
    return out


# ---- 1. generate() against the reference's per-step outputs -----------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(TO.CASES))
def test_generate_against_reference_steps(tag, gold):
    """every case, every step, every layer: the device generates the fixture's ids, then its attentions and hidden states agree with
    the reference's within 8 floors on the live steps and are exactly zero on the steps past a row's end"""
    f, g, (cond, codes) = fixture_gpt(tag, gold)
    sh, dims = TO.SHAPES[tag], TO.case_dims(tag)
    n, L = sh["steps"], dims["n_layer"]
    lengths = torch.from_numpy(f["lengths"])
    assert lengths.tolist() == TO.lengths_of(f["tokens"], dims["stop_audio_token"]).tolist()
    assert (not sh["ragged"]) or int(lengths.min()) < n, "the ragged case must end one row early"
    peak = TO.stored_peak_median([[f[f"att_{i}"][l] for l in range(L)] for i in range(n)], lengths)
    print(f"trace_{tag}: per-layer median of max_k p * keys {peak}")
    assert min(peak) >= TO.MIN_PEAK
    out = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False, max_new_tokens=n, **ASK)
    assert np.array_equal(out.sequences.cpu().numpy(), f["tokens"]), "the device generated other ids than the reference"
    P, cs = N_COND + sh["Tc"] + 2, int(f["channel_step"])
    assert len(out.attentions) == n and len(out.hidden_states) == n
    worst_a = worst_h = 0.0
    for i in range(n):
        assert len(out.attentions[i]) == L and len(out.hidden_states[i]) == L + 1
        a = torch.stack([t.cpu() for t in out.attentions[i]])                       # [L,B,H,rows,keys]
        h = torch.stack([t.cpu() for t in out.hidden_states[i]])[..., ::cs]          # [L+1,B,rows,channels]
        ra, rh = torch.from_numpy(f[f"att_{i}"]), torch.from_numpy(f[f"hid_{i}"])
        assert a.shape == ra.shape and h.shape == rh.shape, (i, a.shape, ra.shape, h.shape, rh.shape)
        assert a.shape[-2:] == ((P + 1, P + 1) if i == 0 else (1, P + 1 + i))
        live = lengths > i
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(h).all())
        assert float(a[:, ~live].abs().max() if bool((~live).any()) else 0.0) == 0.0, f"step {i}: a finished row's attention is not zero"
        assert float(h[:, ~live].abs().max() if bool((~live).any()) else 0.0) == 0.0, f"step {i}: a finished row's hidden state is not zero"
        worst_a = max(worst_a, float((a - ra)[:, live].abs().max()))
        worst_h = max(worst_h, float((h - rh)[:, live].abs().max()))
    fa, fh = float(f["floor_att"]), float(f["floor_hid"])
    print(f"trace_{tag}: attentions max abs err {worst_a:.3e} = {worst_a / fa:.2f} floors ({fa:.3e}); hidden states {worst_h:.3e} = "
          f"{worst_h / fh:.2f} floors ({fh:.3e}); margin {MARGIN}")
    assert worst_a <= MARGIN * fa, f"attentions: {worst_a:.3e} > {MARGIN} x {fa:.3e}"
    assert worst_h <= MARGIN * fh, f"hidden states: {worst_h:.3e} > {MARGIN} x {fh:.3e}"


# ---- 2. structure, GPT.trace, alignment (the tiny case: ragged lengths, T = 67) ---------------------------------------------------
def test_structure_trace_and_alignment(gold):
    f, g, (cond, codes) = fixture_gpt("tiny", gold)
    sh, dims = TO.SHAPES["tiny"], TO.case_dims("tiny")
    n, L, H = sh["steps"], dims["n_layer"], dims["n_head"]
    P = N_COND + sh["Tc"] + 2
    T = P + n
    lengths = torch.from_numpy(f["lengths"])
    cd, kd = cond.to(DEV), codes.to(DEV)
    out = g.generate(cd, kd, do_sample=False, max_new_tokens=n, **ASK)
    tr = g.trace(cd, kd, out.sequences, output_hidden_states=True)
    assert tuple(tr.attentions.shape) == (L, sh["B"], H, T, T) and tuple(tr.hidden_states.shape) == (L + 1, sh["B"], T, dims["d_model"])
    assert tuple(tr.alignment.shape) == (sh["B"], n, sh["Tc"])
    # GPT.trace on the generated ids: the bits generate() returned
    for i in range(n):
        lo, hi = (0 if i == 0 else P + i), P + i + 1
        for l in range(L):
            assert torch.equal(out.attentions[i][l], tr.attentions[l][:, :, lo:hi, :hi]), (i, l)
        for l in range(L + 1):
            assert torch.equal(out.hidden_states[i][l], tr.hidden_states[l][:, lo:hi]), (i, l)
    pr = tr.attentions.cpu()
    assert bool(torch.isfinite(pr).all())
    # exactly zero above the diagonal and on the rows past a finished item's end; the live rows sum to 1
    above = torch.arange(T).view(1, T) > torch.arange(T).view(T, 1)
    assert float(pr[..., above].abs().max()) == 0.0
    dead = torch.arange(T).view(1, T) >= (P + lengths.view(-1, 1))                   # [B,T]
    assert bool(dead.any()) and float(pr.permute(1, 3, 0, 2, 4)[dead].abs().max()) == 0.0
    assert float(tr.hidden_states.cpu().permute(1, 2, 0, 3)[dead].abs().max()) == 0.0
    sums = pr.double().sum(-1).permute(1, 3, 0, 2)[~dead]
    print(f"row sums of the live rows: max |sum - 1| {float((sums - 1).abs().max()):.3e}")
    assert float((sums - 1).abs().max()) <= 1e-6
    # alignment = the head / layer mean of the returned attentions over the content columns, within the rounding of an fp32 sum of
    # H * L terms <= 1 and one multiplication: (H * L + 1) * 2^-24
    want = TO.alignment(pr, P, n, N_COND, sh["Tc"])
    err = float((tr.alignment.cpu().double() - want).abs().max())
    bound = (H * L + 1) * 2.0 ** -24
    print(f"alignment against the mean of the attentions: max abs err {err:.3e} (bound {bound:.3e}); largest row mass "
          f"{float(tr.alignment.sum(-1).max()):.4f}")
    assert err <= bound and float(tr.alignment.sum(-1).max()) <= 1.0 + 1e-6
    again = g.trace(cd, kd, out.sequences, output_hidden_states=True)
    assert torch.equal(again.alignment, tr.alignment) and torch.equal(again.attentions, tr.attentions)
    assert torch.equal(again.hidden_states, tr.hidden_states)
    # without the L-fold tensor (one layer's scratch): the same alignment bits; a layer choice: that layer's head mean
    lean = g.trace(cd, kd, out.sequences, output_attentions=False)
    assert lean.attentions is None and lean.hidden_states is None and torch.equal(lean.alignment, tr.alignment)
    last = g.trace(cd, kd, out.sequences, output_attentions=False, alignment_layers=[-1])
    err = float((last.alignment.cpu().double() - TO.alignment(pr, P, n, N_COND, sh["Tc"], layers=[L - 1])).abs().max())
    assert err <= (H + 1) * 2.0 ** -24, err
    # explicit lengths: a shorter length zeroes more steps
    short = g.trace(cd, kd, out.sequences, code_lengths=[3, 5], output_hidden_states=True)
    assert float(short.attentions[:, 0, :, P + 3:].abs().max()) == 0.0 and float(short.attentions[:, 1, :, P + 5:].abs().max()) == 0.0
    assert torch.equal(short.attentions[:, 1, :, :P + 5], tr.attentions[:, 1, :, :P + 5])
    with pytest.raises(ValueError, match="length"):
        g.trace(cd, kd, out.sequences, code_lengths=[0, 5])


# ---- 3. default weights and the peaked preset of 20, against the float64 oracle -----------------------------------------------------
def test_default_and_peaked20_against_float64():
    """default synthetic weights: hidden states within the 1e-4 absolute of the teacher-forced latent tests.  act_stats' `peaked` preset
    (score std 20, score ranges past 88: exp overflows without the maximum subtracted, whole key tiles underflow): every value finite
    and within act_stats.yardstick's rule of the float64 oracle, on the device's own greedy ids"""
    tag, seed = "tiny", 7
    dims, sh = TO.case_dims(tag), TO.SHAPES[tag]
    cond, codes = TO.case_inputs(tag, seed)
    n = 24
    res = {}
    for preset in ("default", "peaked"):
        w = weights(tag, seed, None, preset)
        g = make_gpt(tag, w)
        out = g.generate(cond.to(DEV), codes.to(DEV), do_sample=False, max_new_tokens=n, return_dict_in_generate=True)
        ids = out.sequences.cpu()
        lengths = TO.lengths_of(ids, dims["stop_audio_token"])
        tr = g.trace(cond.to(DEV), codes.to(DEV), out.sequences, output_hidden_states=True)
        with act_stats.record() as st:
            p32, h32, p64, h64, _, _ = floors(w, dims, cond, codes, ids, lengths)
        if preset == "peaked":
            act_stats.check_regime("peaked", st, "trace")
        pk, hk = tr.attentions.cpu(), tr.hidden_states.cpu()
        assert bool(torch.isfinite(pk).all()) and bool(torch.isfinite(hk).all())
        res[preset] = (pk, hk, p32, h32, p64, h64)
    pk, hk, p32, h32, p64, h64 = res["default"]
    err = act_stats.maxdev(hk, h64)
    print(f"default weights: hidden states max abs err against float64 {err:.3e} (1e-4), attentions {act_stats.maxdev(pk, p64):.3e}")
    assert err <= 1e-4
    qk, gk, q32, g32, q64, g64 = res["peaked"]
    act_stats.yardstick("peaked-20 attentions", qk, q64, q32, pk, p64)
    act_stats.yardstick("peaked-20 hidden states", gk, g64, g32, hk, h64)
    sums = qk.double().sum(-1)
    live = sums > 0
    assert float((sums[live] - 1).abs().max()) <= 1e-6


# ---- 4. sampling with num_return_sequences, guidance: against the oracle on the device's own ids ---------------------------------
def _against_oracle(what, out, w, dims, cond, codes, P):
    ids = out.sequences.cpu()
    n = ids.shape[1]
    lengths = TO.lengths_of(ids, dims["stop_audio_token"])
    p32, h32, p64, h64, fa, fh = floors(w, dims, cond, codes, ids, lengths)
    L, rows, H, T = p32.shape[:4]
    pk = stack_steps(out.attentions, p32.shape, P)
    hk = stack_steps(out.hidden_states, h32.shape, P)
    # what the per-step form does not carry (rows P+1.. of the columns to their right are zero by construction) is zero in the oracle too
    ea, eh = act_stats.maxdev(pk, p64), act_stats.maxdev(hk, h64)
    print(f"{what}: {rows} rows x {n} steps, lengths {lengths.tolist()}: attentions {ea:.3e} = {ea / fa:.2f} floors ({fa:.3e}), hidden "
          f"states {eh:.3e} = {eh / fh:.2f} floors ({fh:.3e})")
    assert ea <= MARGIN * fa and eh <= MARGIN * fh


def test_sampling_num_return_sequences_and_guidance(gold):
    f, g, (cond, codes) = fixture_gpt("tiny", gold)
    sh, dims = TO.SHAPES["tiny"], TO.case_dims("tiny")
    seed, bias = int(f["seed"]), float(f["stop_bias"])
    w = weights("tiny", seed, bias)
    P = N_COND + sh["Tc"] + 2
    cd, kd = cond.to(DEV), codes.to(DEV)
    kw = dict(do_sample=True, top_k=20, temperature=1.0, seed=5, max_new_tokens=20)
    bare = g.generate(cd, kd, num_return_sequences=2, **kw)
    out = g.generate(cd, kd, num_return_sequences=2, **kw, **ASK)
    assert torch.equal(out.sequences, bare) and out.sequences.shape[0] == 4
    _against_oracle("sampling, num_return_sequences=2", out, w, dims, cond.repeat_interleave(2, 0), codes.repeat_interleave(2, 0), P)
    ncond = synth.uniform(seed + 100, "cond_latents", tuple(cond.shape), 1.0)
    gkw = dict(guidance_scale=1.5, negative_cond_latents=ncond.to(DEV), do_sample=False, max_new_tokens=20)
    bare = g.generate(cd, kd, **gkw)
    out = g.generate(cd, kd, **gkw, **ASK)
    assert torch.equal(out.sequences, bare) and out.sequences.shape[0] == 2
    _against_oracle("guidance_scale=1.5 (the conditional rows)", out, w, dims, cond, codes, P)


# ---- 5. the kwargs change no token and run nothing unless asked for; bf16 contexts refuse -------------------------------------------
def test_tokens_unchanged_and_no_new_code_unless_asked(gold, monkeypatch):
    f, g, (cond, codes) = fixture_gpt("tiny", gold)
    cd, kd = cond.to(DEV), codes.to(DEV)
    for kw in (dict(do_sample=False, max_new_tokens=24), dict(do_sample=True, top_k=50, seed=3, max_new_tokens=16)):
        bare = g.generate(cd, kd, **kw)
        assert torch.equal(g.generate(cd, kd, **kw, **ASK).sequences, bare)
    # the plain call -- what bench.py times -- and a call whose kwargs HF ignores never reach the trace pass
    def boom(*a, **k):
        raise AssertionError("engine.trace reached without output_attentions / output_hidden_states being asked for")
    monkeypatch.setattr(g.engine, "trace", boom)
    kw = dict(do_sample=False, max_new_tokens=24)
    bare = g.generate(cd, kd, **kw)
    assert torch.equal(g.generate(cd, kd, output_attentions=True, output_hidden_states=True, **kw), bare)
    out = g.generate(cd, kd, return_dict_in_generate=True, output_scores=True, **kw)
    assert torch.equal(out.sequences, bare) and "attentions" not in out
    with pytest.raises(AssertionError, match="engine.trace reached"):
        g.generate(cd, kd, **kw, **ASK)


def test_bf16_context_refuses(gold):
    f = gold("trace_tiny")
    seed = int(f["seed"])
    g = make_gpt("tiny", weights("tiny", seed, float(f["stop_bias"])), weight_dtype="bf16_kv")
    cond, codes = TO.case_inputs("tiny", seed)
    cd, kd = cond.to(DEV), codes.to(DEV)
    with pytest.raises(NotImplementedError, match="bf16_kv"):
        g.generate(cd, kd, do_sample=False, max_new_tokens=8, **ASK)
    ids = g.generate(cd, kd, do_sample=False, max_new_tokens=8)
    with pytest.raises(NotImplementedError, match="bf16_kv"):
        g.trace(cd, kd, ids)
    # the library itself refuses (GVC_ERR_UNSUPPORTED), whatever the Python layer checked
    prefix = g.engine.prefix_embeddings(cd, kd.int())
    with pytest.raises(NotImplementedError, match="bf16_kv"):
        g.engine.trace(torch.arange(2, device=DEV, dtype=torch.int32), prefix, ids.int(), [8, 8], N_COND)
