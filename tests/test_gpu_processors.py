"""GPU: the length / repetition logits processors (include/genvc_hip.h: gvc_logits_processors) against
tests/golden/logits_processors.npz (the reference's sample_stream / GPT.generate with the installed transformers' processors, executed:
scripts/make_processor_golden.py) on every decode path, min_p against HF's kept set and probabilities, the all-default invariant and the
warm path."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proc_oracle as PO                      # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logits_processors.npz")
EOS, V = 1025, 1026
GREEDY = dict(do_sample=True, top_k=1, top_p=1.0, temperature=1.0, repetition_penalty=2.0)


def greedy(gold, tag):
    """the fixture case's greedy settings (its repetition penalty: 1.0 for the n-gram cases, 2.0 otherwise)"""
    return dict(GREEDY, repetition_penalty=float(gold[f"{tag}_rep"]))


def make_gpt(model_args, seed, stop_bias=None, max_slots=16):
    from genvc_amd.layers.gpt import GPT
    a = model_args
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    dims = gcfg.gpt_dims(a)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][EOS] = float(stop_bias)
    g.load_state_dict(w, strict=False)
    g.to(DEV)
    g.init_gpt_for_inference(max_slots=max_slots)
    return g, dims


def load_case(gold, tag):
    full = bool(gold[f"{tag}_full"])
    sb = float(gold[f"{tag}_stop_bias"])
    g, dims = make_gpt(gcfg.DEFAULT_MODEL_ARGS if full else gcfg.TINY_MODEL_ARGS, int(gold[f"{tag}_seed"]),
                       stop_bias=sb if sb != 0.0 else None)
    g.case_weights = (synth.make_weights(int(gold[f"{tag}_seed"]), synth.gpt_weight_spec(dims)), dims)
    g.max_gen_mel_tokens = int(gold[f"{tag}_max_new"])
    B, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(s, "content_codes", (B, Tc), 256).to(DEV)
    kw = json.loads(str(gold[f"{tag}_kw"]))
    if "exponential_decay_length_penalty" in kw:
        kw["exponential_decay_length_penalty"] = tuple(kw["exponential_decay_length_penalty"])
    return g, cond, codes, kw


def trim(toks):
    """a row's tokens up to and including its first stop token (the reference loop of a lone row ends there)"""
    hit = np.nonzero(toks == EOS)[0]
    return toks[:int(hit[0]) + 1] if len(hit) else toks


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def cases(gold, kind):
    return [t for t in json.loads(str(gold["cases"])) if str(gold[f"{t}_kind"]) == kind]


def _close(g):
    g.engine.close()
    del g
    torch.cuda.empty_cache()


# ---- 1. GPT.generate: every sampler case at B = 1 and at the fixture's B, on both decode classes --------------------------------
@pytest.mark.parametrize("one_launch", ["1", "0"], ids=["one_launch_steps", "launch_per_phase"])
def test_generate_matches_executed_reference(gold, one_launch, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST", one_launch)
    monkeypatch.setenv("GVC_PERSIST_ROWS", one_launch)
    for tag in cases(gold, "sampler"):
        g, cond, codes, kw = load_case(gold, tag)
        want = gold[f"{tag}_tokens"]
        got = g.generate(cond, codes, group=8, **greedy(gold, tag), **kw).cpu().numpy()
        assert np.array_equal(got, want), tag
        one = g.generate(cond[:1], codes[:1], group=8, **greedy(gold, tag), **kw).cpu().numpy()
        assert np.array_equal(one[0], trim(want[0])), tag
        # without the processors the call returns the baseline the fixture was screened against
        base = g.generate(cond, codes, group=8, **greedy(gold, tag)).cpu().numpy()
        assert np.array_equal(base, gold[f"{tag}_base"]), tag
        _close(g)


# ---- 2. get_generator: streamed pairs, latents against the teacher-forced re-pass ----------------------------------------------
def test_get_generator_matches_executed_reference(gold):
    for tag in cases(gold, "sampler"):
        g, cond, codes, kw = load_case(gold, tag)
        want = gold[f"{tag}_tokens"]
        fake = g.compute_embeddings(cond, codes)
        pairs = list(g.get_generator(fake_inputs=fake, stream_group=8, **greedy(gold, tag), **kw))
        toks = torch.stack([p[0] for p in pairs], 1).cpu().numpy()
        lats = torch.stack([p[1] for p in pairs], 1)
        assert np.array_equal(toks, want), tag
        # the latents of row 0 against the re-pass of its generated codes (inference_utils.py:68-76)
        gen = torch.from_numpy(trim(want[0]))
        gen = gen[gen != EOS].unsqueeze(0).to(DEV)
        Tc = codes.shape[1]
        rel = g(codes[:1], torch.tensor([Tc], device=DEV), gen, torch.tensor([gen.shape[1] * 1024], device=DEV),
                cond_latents=cond[:1], return_latent=True)
        np.testing.assert_allclose(rel[0].cpu().numpy(), lats[0, :gen.shape[1]].cpu().numpy(), atol=1e-4)
        _close(g)


# ---- 3. generate_groups / generate_rolling (greedy): rows counted from their own prompts ----------------------------------------
def test_groups_and_rolling_match_executed_reference(gold):
    for tag in cases(gold, "sampler"):
        g, cond, codes, kw = load_case(gold, tag)
        want = gold[f"{tag}_tokens"]
        B = cond.shape[0]
        if B == 1:
            _close(g)
            continue
        rep = float(gold[f"{tag}_rep"])
        # The second group gets a shorter prompt (fewer code tokens), so the rows of one joint decode have different prompt lengths.
        # Its expected tokens come from the CPU restatement, margin-screened like the fixture: the first cut whose screen passes is
        # used, and a case where none does fails here rather than going unchecked.
        w, dims = g.case_weights
        sb = float(gold[f"{tag}_stop_bias"])
        if sb != 0.0:
            w["mel_head.bias"][EOS] = sb
        ora = PO.BO.OracleGpt(w, dims)
        for cut in (2, 4, 3, 6, 1, 5):
            short = codes[:, :codes.shape[1] - cut].contiguous()
            solo, gaps = PO.greedy(ora, cond[1:].cpu(), short[1:].cpu(), kw, rep, int(gold[f"{tag}_max_new"]))
            if gaps[np.isfinite(gaps)].min() >= 2e-3:
                break
        else:
            pytest.fail(f"{tag}: no shorter prompt passes the margin screen")
        solo = solo[:, :max(len(trim(r)) for r in solo)]
        groups = [(cond[:1], codes[:1]), (cond[1:], short[1:])]
        g.groups_stats = {"joint": 0, "separate": 0}
        outs = g.generate_groups(groups, group=8, **greedy(gold, tag), **kw)
        assert g.groups_stats["joint"] == 1
        assert np.array_equal(outs[0].cpu().numpy()[0], trim(want[0])), tag
        assert np.array_equal(outs[1].cpu().numpy(), solo), (tag, cut)
        jobs = groups + [(cond[B - 1:], codes[B - 1:])]
        outs = g.generate_rolling(jobs, group=8, max_rows=2, **greedy(gold, tag), **kw)
        assert np.array_equal(outs[0].cpu().numpy()[0], trim(want[0])), tag
        assert np.array_equal(outs[1].cpu().numpy(), solo), (tag, cut)
        assert np.array_equal(outs[2].cpu().numpy()[0], trim(want[B - 1])), tag
        _close(g)


# ---- 4. beams at K = 2 and 4 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_launch", ["1", "0"], ids=["one_launch_steps", "launch_per_phase"])
def test_beams_match_executed_reference(gold, one_launch, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST_ROWS", one_launch)
    seen = set()
    for tag in cases(gold, "beam"):
        g, cond, codes, kw = load_case(gold, tag)
        K = int(gold[f"{tag}_K"])
        seen.add(K)
        ids = g.generate(cond, codes, num_beams=K, do_sample=False, length_penalty=float(gold[f"{tag}_lp"]),
                         repetition_penalty=float(gold[f"{tag}_rep"]),
                         beam_length_mode="generated", group=8, **kw)
        assert np.array_equal(ids.cpu().numpy(), gold[f"{tag}_tokens"]), tag
        np.testing.assert_allclose(g.last_beam_scores.numpy(), gold[f"{tag}_best_scores"], rtol=1e-4, atol=1e-5)
        _close(g)
    assert seen == {2, 4}


# ---- 5. min_p with temperature, top-k and top-p through the sampler entry point --------------------------------------------------
def _hf_probs(s, temperature, top_k, top_p, min_p):
    from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    x = s[None].clone()
    # (the warpers _get_logits_processor builds for these settings: top-k only when > 0, top-p only when < 1)
    warpers = [TemperatureLogitsWarper(temperature)] + ([TopKLogitsWarper(top_k)] if top_k > 0 else []) + \
        ([TopPLogitsWarper(top_p)] if top_p < 1.0 else []) + [MinPLogitsWarper(min_p)]
    for p in warpers:
        x = p(None, x)
    return torch.softmax(x[0], -1)


@pytest.mark.parametrize("temperature,top_k,top_p,min_p", [(0.8, 50, 0.95, 0.1), (1.3, 0, 1.0, 0.05), (0.7, 200, 0.9, 0.3)])
def test_min_p_draws_follow_hf(temperature, top_k, top_p, min_p):
    from genvc_amd.engine import GptEngine, logits_processors, sample_params
    gen = torch.Generator().manual_seed(7)
    s = torch.randn(V, generator=gen) * 2.0
    p_hf = _hf_probs(s, temperature, top_k, top_p, min_p)
    kept = p_hf > 0
    assert 2 <= int(kept.sum()) < int((_hf_probs(s, temperature, top_k, top_p, 0.0) > 0).sum())      # min_p drops ids here
    B, n0, steps = 64, 8, 80
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    eng = GptEngine(dims, max_slots=4)
    params = sample_params(dict(repetition_penalty=1.0, temperature=temperature, top_p=top_p, top_k=top_k), V, EOS, seed=11)
    proc = logits_processors(dict(min_p=min_p), n0, V)
    logits = s.to(DEV).expand(B, V).contiguous()
    counts = torch.zeros(V, dtype=torch.long)
    for step in range(steps):
        ids = torch.ones(B, n0 + 2, device=DEV, dtype=torch.int32)
        ids[:, n0 - 1] = 1024
        ids_len = torch.full((B,), n0, device=DEV, dtype=torch.int32)
        fin = torch.zeros(B, device=DEV, dtype=torch.int32)
        tok = eng.sample_proc(logits, ids, ids_len, fin, params, proc, step)
        counts += torch.bincount(tok.long().cpu(), minlength=V)
    n = B * steps
    assert int(counts[~kept].sum()) == 0, "a draw outside HF's kept set"
    exp = p_hf.double() * n
    obs = counts.double()
    big = exp >= 5
    stat = float(((obs[big] - exp[big]) ** 2 / exp[big]).sum())
    rest_e, rest_o = float(exp[~big & kept].sum()), float(obs[~big & kept].sum())
    dof = int(big.sum()) - 1
    if rest_e > 0:
        stat += (rest_o - rest_e) ** 2 / rest_e
        dof += 1
    # Wilson-Hilferty: the chi-square quantile at 1 - 1e-4
    z = 3.719
    crit = dof * (1 - 2 / (9 * dof) + z * math.sqrt(2 / (9 * dof))) ** 3
    assert stat < crit, (stat, crit, dof)
    eng.close()


# ---- 6. every setting at its default: bit-identical, on every path; an all-zero struct on the kernels ---------------------------
DEFAULTS = dict(min_new_tokens=0, min_length=0, no_repeat_ngram_size=0, suppress_tokens=None, begin_suppress_tokens=None,
                exponential_decay_length_penalty=None, min_p=None)


def test_defaults_are_bit_identical(gold):
    tag = cases(gold, "sampler")[0]
    g, cond, codes, _ = load_case(gold, tag)
    a = g.generate(cond, codes, **GREEDY)
    la = g.last_latents.clone()
    b = g.generate(cond, codes, **GREEDY, **DEFAULTS)
    assert torch.equal(a, b) and torch.equal(la, g.last_latents)
    samp = dict(do_sample=True, top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0, seed=5)
    a = g.generate(cond, codes, **samp)
    la = g.last_latents.clone()
    b = g.generate(cond, codes, **samp, **DEFAULTS)
    assert torch.equal(a, b) and torch.equal(la, g.last_latents)
    fake = g.compute_embeddings(cond, codes)
    pa = list(g.get_generator(fake_inputs=fake, **GREEDY))
    pb = list(g.get_generator(fake_inputs=fake, **GREEDY, **DEFAULTS))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(pa, pb)) and len(pa) == len(pb)
    groups = [(cond[:1], codes[:1]), (cond[1:], codes[1:])]
    oa = g.generate_groups(groups, **GREEDY)
    ob = g.generate_groups(groups, **GREEDY, **DEFAULTS)
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    oa = g.generate_rolling(groups, max_rows=2, **GREEDY)
    ob = g.generate_rolling(groups, max_rows=2, **GREEDY, **DEFAULTS)
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    beam = dict(num_beams=2, do_sample=False, repetition_penalty=2.0, beam_length_mode="generated")
    a = g.generate(cond[:2], codes[:2], **beam)
    sa = g.last_beam_scores.clone()
    b = g.generate(cond[:2], codes[:2], **beam, **DEFAULTS)
    assert torch.equal(a, b) and torch.equal(sa, g.last_beam_scores)
    _close(g)


@pytest.mark.parametrize("top_k", [1, 15, 0])
def test_all_zero_struct_changes_no_kernel_result(top_k):
    """the kernels themselves: a non-null, all-zero gvc_logits_processors gives the tokens of the call without one"""
    from genvc_amd import _lib
    from genvc_amd.engine import BeamSearch, GptEngine, beam_select, sample_params
    gen = torch.Generator().manual_seed(3 + top_k)
    B, n0 = 5, 9
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    eng = GptEngine(dims, max_slots=4)
    params = sample_params(dict(repetition_penalty=2.0, temperature=0.85, top_p=0.85, top_k=top_k), V, EOS, seed=2)
    zero = _lib.LogitsProcessors()
    for step in range(20):
        logits = (torch.randn(B, V, generator=gen) * 3).to(DEV)
        ids = torch.randint(0, V, (B, n0 + 4), generator=gen).int().to(DEV)
        outs = []
        for proc in (None, zero):
            ids_len = torch.full((B,), n0, device=DEV, dtype=torch.int32)
            fin = torch.zeros(B, device=DEV, dtype=torch.int32)
            i2 = ids.clone()
            outs.append(eng.sample(logits, i2, ids_len, fin, params, step) if proc is None else
                        eng.sample_proc(logits, i2, ids_len, fin, params, proc, step))
        assert torch.equal(outs[0], outs[1]), step
    fake = torch.randint(0, 1024, (2, n0), generator=gen)
    bs = [BeamSearch(fake.to(DEV), 4, 6, EOS, V, 1.0, 2.0, "generated", proc=p) for p in (None, zero)]
    sl = [torch.arange(8, device=DEV, dtype=torch.int32) for _ in bs]
    for t in range(5):
        logits = (torch.randn(8, V, generator=gen) * 3).to(DEV)
        for beam, s in zip(bs, sl):
            beam_select(beam, logits, s, t)
            beam.steps = t + 1
        assert torch.equal(bs[0].tokens, bs[1].tokens) and torch.equal(bs[0].scores, bs[1].scores) and torch.equal(sl[0], sl[1])
    eng.close()


# ---- 7. warm path: a processor-carrying call neither allocates nor captures -------------------------------------------------------
def test_processor_calls_after_warmup_neither_allocate_nor_capture(gold):
    tag = cases(gold, "sampler")[0]
    g, cond, codes, kw = load_case(gold, tag)
    eng = g.engine
    B = cond.shape[0]
    n0 = 32 + codes.shape[1] + 3
    mx = n0 + g.max_gen_mel_tokens
    eng.warmup(B, mx, 1)
    eng.warmup_range(B, n0 + 1, mx, 1)
    eng.warmup_beam(2, 2, mx)
    g.generate(cond, codes, **GREEDY)
    base = eng.lazy_inits()
    g.generate(cond, codes, **GREEDY, **kw)
    g.generate(cond, codes, **GREEDY, no_repeat_ngram_size=3, suppress_tokens=[5], exponential_decay_length_penalty=(5, 1.1))
    g.generate(cond[:2], codes[:2], num_beams=2, do_sample=False, repetition_penalty=2.0, min_new_tokens=4, no_repeat_ngram_size=2)
    torch.cuda.synchronize()
    assert eng.lazy_inits() == base
    _close(g)


# ---- 8. the documented deviation: EOS banned (min_new_tokens) while the decay applies stays banned ------------------------------------
def test_banned_eos_stays_banned_under_the_decay():
    """HF computes -inf + inf = NaN for EOS there; the device keeps it -inf: EOS is never drawn while banned, and is the
    argmax once the ban has lifted"""
    from genvc_amd.engine import GptEngine, logits_processors, sample_params
    B, n0 = 4, 8
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    eng = GptEngine(dims, max_slots=4)
    gen = torch.Generator().manual_seed(5)
    logits = torch.randn(B, V, generator=gen)
    logits[:, EOS] = -0.5                      # the top score, negative: the decay raises it, it cannot lower it below the others
    logits = logits.clamp(max=-0.6)
    logits[:, EOS] = -0.5
    logits = logits.to(DEV).contiguous()
    proc = logits_processors(dict(min_new_tokens=3, exponential_decay_length_penalty=(0, 2.0)), n0, V)
    for top_k in (1, 15):
        params = sample_params(dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=top_k), V, EOS, seed=1)
        for new in range(5):
            ids = torch.ones(B, n0 + 8, device=DEV, dtype=torch.int32)
            ids_len = torch.full((B,), n0 + new, device=DEV, dtype=torch.int32)
            fin = torch.zeros(B, device=DEV, dtype=torch.int32)
            tok = eng.sample_proc(logits, ids, ids_len, fin, params, proc, new).cpu()
            if new < 3:
                assert not bool((tok == EOS).any()), (top_k, new)          # banned: HF's NaN would make greedy pick EOS here
            elif top_k == 1:
                assert bool((tok == EOS).all()), new
    eng.close()
