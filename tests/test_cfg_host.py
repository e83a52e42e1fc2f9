"""CPU: classifier-free guidance (GPT.generate(guidance_scale=...)): the validation and dispatch of the kwargs on a CPU-constructed GPT,
the paths that refuse guidance by name, the closed-form combine of tests/cfg_oracle.py against the installed transformers'
UnbatchedClassifierFreeGuidanceLogitsProcessor (executed), infer.py's flags, and the new C ABI symbols."""
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cfg_oracle as CF                       # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gvc_cfg_guide", "gvc_gpt_generate_cfg", "gvc_gpt_warmup_cfg")
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]


def cpu_gpt(max_slots=8):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"])
    g.max_slots = max_slots
    return g


def inputs(B=2, Tc=5):
    return torch.zeros(B, 32, D), torch.zeros(B, Tc, dtype=torch.long)


def test_guidance_scale_parsing():
    from genvc_amd.layers.gpt import _guidance_scale
    assert _guidance_scale({}) is None
    assert _guidance_scale(dict(guidance_scale=None)) is None
    assert _guidance_scale(dict(guidance_scale=1)) is None and _guidance_scale(dict(guidance_scale=1.0)) is None
    assert _guidance_scale(dict(guidance_scale=1.5)) == 1.5
    assert _guidance_scale(dict(guidance_scale=3)) == 3.0
    assert _guidance_scale(dict(guidance_scale=0.5)) == 0.5
    for bad in (float("nan"), float("inf"), float("-inf"), True, False, "strong"):
        with pytest.raises(ValueError, match="guidance_scale"):
            _guidance_scale(dict(guidance_scale=bad))


def test_missing_negative_raises_value_error():
    """guidance on without negative_cond_latents: HF's default unconditional prompt (the bare last token) means nothing here.  Before
    guidance existed the kwarg was ignored and the call went on to the engine check (RuntimeError)."""
    g = cpu_gpt()
    cond, codes = inputs()
    with pytest.raises(ValueError, match="negative_cond_latents"):
        g.generate(cond, codes, guidance_scale=1.5, do_sample=False)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), True])
def test_bad_scale_raises_value_error(bad):
    g = cpu_gpt()
    cond, codes = inputs()
    with pytest.raises(ValueError, match="guidance_scale"):
        g.generate(cond, codes, guidance_scale=bad, negative_cond_latents=cond)


def test_negative_shapes_and_slots():
    g = cpu_gpt()
    cond, codes = inputs(B=2)
    with pytest.raises(ValueError, match="negative_cond_latents must be"):
        g.generate(cond, codes, guidance_scale=1.5, negative_cond_latents=torch.zeros(3, 32, D))          # leading dim not in {1, B}
    with pytest.raises(ValueError, match="negative_cond_latents must be"):
        g.generate(cond, codes, guidance_scale=1.5, negative_cond_latents=torch.zeros(2, 32, D + 1))      # wrong d
    with pytest.raises(ValueError, match="negative_cond_latents must be"):
        g.generate(cond, codes, guidance_scale=1.5, negative_cond_latents=torch.zeros(32, D))
    with pytest.raises(ValueError, match="negative_text_inputs must be"):
        g.generate(cond, codes, guidance_scale=1.5, negative_cond_latents=cond, negative_text_inputs=torch.zeros(3, 4, dtype=torch.long))
    g5 = cpu_gpt(max_slots=3)
    with pytest.raises(ValueError, match=re.escape("init_gpt_for_inference(max_slots=")):
        g5.generate(cond, codes, guidance_scale=1.5, negative_cond_latents=cond)
    # a valid guided call, broadcasting negatives included, gets as far as the engine check (no engine on this CPU-only module)
    for neg, negt in ((cond, None), (cond[:1], None), (cond, codes[:1, :3]), (cond[:1], torch.zeros(2, 9, dtype=torch.long))):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate(cond, codes, guidance_scale=1.5, negative_cond_latents=neg, negative_text_inputs=negt)


def test_combinations_raise_by_name():
    g = cpu_gpt(max_slots=16)
    cond, codes = inputs(B=1)
    base = dict(guidance_scale=2.0, negative_cond_latents=cond)
    with pytest.raises(NotImplementedError, match=r"guidance_scale=2\.0 with beam search \(num_beams=4\)"):
        g.generate(cond, codes, num_beams=4, do_sample=False, **base)
    with pytest.raises(NotImplementedError, match=r"guidance_scale=2\.0 with beam groups"):
        g.generate(cond, codes, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, do_sample=False, **base)
    with pytest.raises(NotImplementedError, match=r"guidance_scale=2\.0 with contrastive search"):
        g.generate(cond, codes, do_sample=False, top_k=4, penalty_alpha=0.6, **base)
    with pytest.raises(NotImplementedError, match=r"guidance_scale=2\.0 with num_return_sequences=3"):
        g.generate(cond, codes, num_return_sequences=3, **base)
    # the combinations are refused before the missing negative is
    with pytest.raises(NotImplementedError, match="beam search"):
        g.generate(cond, codes, num_beams=4, do_sample=False, guidance_scale=2.0)


def test_refused_paths_name_themselves():
    from genvc_amd.streaming import StreamSessions
    g = cpu_gpt()
    cond, codes = inputs(B=1)
    kw = dict(guidance_scale=1.5, negative_cond_latents=cond)
    with pytest.raises(NotImplementedError, match=re.escape("guidance_scale=1.5) is not on the streaming (get_generator) path")):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))
    with pytest.raises(NotImplementedError, match=re.escape("guidance_scale=1.5) is not on the grouped (generate_groups) path")):
        g.generate_groups([(cond, codes)], **kw)
    with pytest.raises(NotImplementedError, match=re.escape("guidance_scale=1.5) is not on the rolling (generate_rolling) path")):
        g.generate_rolling([(cond, codes)], **kw)
    with pytest.raises(NotImplementedError, match=re.escape("guidance_scale=1.5) is not on the session (StreamSessions, open) path")):
        StreamSessions._procs(object(), dict(guidance_scale=1.5), {}, "open")
    # guidance off: these paths behave as before (they reach the engine check; a bad scale is still a ValueError)
    for off in (dict(guidance_scale=1.0, negative_cond_latents=cond), dict(guidance_scale=None), {}):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **off))
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate_groups([(cond, codes)], **off)
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate_rolling([(cond, codes)], top_k=1, **off)
    with pytest.raises(ValueError, match="guidance_scale"):
        g.generate_groups([(cond, codes)], guidance_scale=float("nan"))


@pytest.mark.parametrize("off", [dict(guidance_scale=1.0), dict(guidance_scale=1), dict(guidance_scale=None), {}])
def test_guidance_off_reaches_the_existing_path_unchanged(off, monkeypatch):
    """guidance_scale None or 1: the sampling path gets the caller's kwargs as they are, negative_* included and ignored (HF ignores
    negative_prompt_ids then), and no guided state"""
    g = cpu_gpt()
    cond, codes = inputs()
    seen = {}

    class Reached(Exception):
        pass

    def start(fake, kw, fan=1):
        seen.update(kw)
        seen["fan"] = fan
        raise Reached

    monkeypatch.setattr(g, "compute_embeddings", lambda c, t: torch.ones(int(t.shape[0]), 40, dtype=torch.long))
    monkeypatch.setattr(g, "_start", start)
    monkeypatch.setattr(g, "_generate_guided", lambda *a, **k: pytest.fail("guided branch taken with guidance off"))
    kw = dict(do_sample=False, repetition_penalty=2.0, max_new_tokens=7, negative_cond_latents=cond, **off)
    with pytest.raises(Reached):
        g.generate(cond, codes, **kw)
    assert seen.pop("fan") == 1
    assert set(seen) == set(kw) and all(seen[k] is kw[k] for k in kw)


@pytest.mark.parametrize("scale", [0.5, 1.5, 3.0, -1.0])
def test_closed_form_equals_the_executed_hf_class(scale):
    gen = torch.Generator().manual_seed(11)
    for B, mag in ((1, 10.0), (3, 10.0), (3, 300.0)):
        cond = (torch.rand(B, 1026, generator=gen) * 2 - 1) * mag
        uncond = (torch.rand(B, 1026, generator=gen) * 2 - 1) * mag
        want = CF.hf_combine(cond, uncond, scale)
        assert torch.equal(CF.closed_form(cond, uncond, scale), want)
        assert torch.isfinite(want).all()
    # cond == uncond: the guided scores are log_softmax(cond), whatever the scale
    assert torch.equal(CF.hf_combine(cond, cond, scale), torch.log_softmax(cond, -1))


def test_hf_puts_the_guidance_processor_first():
    """the order the device restates: transformers builds the guidance processor ahead of every other one"""
    from transformers import GenerationConfig, GenerationMixin
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor
    cfg = GenerationConfig(eos_token_id=1025, pad_token_id=1025, guidance_scale=1.5, repetition_penalty=2.0, no_repeat_ngram_size=2,
                           min_new_tokens=6, do_sample=False, top_k=None, top_p=None, temperature=None)
    cfg._eos_token_tensor = torch.tensor([1025])

    class _M:
        config = type("C", (), {"is_encoder_decoder": False})()
        _merge_criteria_processor_list = GenerationMixin._merge_criteria_processor_list

        def __call__(self, *a, **k):
            raise AssertionError("not run")
    procs = GenerationMixin._get_logits_processor(_M(), generation_config=cfg, input_ids_seq_length=40, encoder_input_ids=None,
                                                  logits_processor=None, device="cpu", model_kwargs={})
    assert isinstance(procs[0], UnbatchedClassifierFreeGuidanceLogitsProcessor)
    assert [type(p).__name__ for p in procs[1:]] == ["RepetitionPenaltyLogitsProcessor", "NoRepeatNGramLogitsProcessor",
                                                     "MinNewTokensLengthLogitsProcessor"]


def _infer(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--device", "cpu", *flags], capture_output=True, text=True,
                          env=env, cwd=ROOT)


def test_infer_flags():
    r = _infer("--streaming", "--guidance_scale", "1.5")
    assert r.returncode != 0 and "--guidance_scale is not on the streaming path (--streaming)" in r.stderr
    r = _infer("--guidance_scale", "nan")
    assert r.returncode != 0 and "--guidance_scale must be finite" in r.stderr
    r = _infer("--guidance_scale", "2.0", "--num_beams", "4")
    assert r.returncode != 0 and "does not combine" in r.stderr
    r = _infer("--negative_ref_audio", "x.wav")
    assert r.returncode != 0 and "--negative_ref_audio needs --guidance_scale" in r.stderr
    # guidance off (1) passes the flag checks with --streaming: the run then fails on the missing checkpoint, not on the flags
    r = _infer("--streaming", "--guidance_scale", "1.0", "--model_path", os.path.join(ROOT, "no_such_checkpoint.pth"))
    assert r.returncode != 0 and "guidance_scale" not in r.stderr


def test_harness_passes_guidance_through(monkeypatch):
    """synthesize_utt computes the negative latents once per utterance (default: the source itself, resampled to the conditioning
    rate) and hands them to every segment's generate call; with guidance off nothing is computed or passed"""
    from genvc_amd.inference import inference_utils as IU
    calls = dict(cond=[], gen=[], resample=[])

    class M:
        device = "cpu"
        content_sample_rate = 16000
        hifigan = None
        config = type("C", (), dict(audio=type("A", (), dict(sample_rate=24000))(), top_p=0.85, top_k=15, temperature=0.75,
                                    length_penalty=1.0, repetition_penalty=10.0,
                                    model_args=type("MA", (), dict(gpt_code_stride_len=1024))()))()

        def get_gpt_cond_latents(self, audio, sr):
            calls["cond"].append((tuple(audio.shape), sr))
            return torch.full((1, 32, D), float(len(calls["cond"])))

        class content_extractor:
            @staticmethod
            def extract_content_features(seg):
                return torch.zeros(1, 4, 8)

        class content_dvae:
            @staticmethod
            def get_codebook_indices(feat):
                return torch.zeros(1, 4, dtype=torch.long)

        class gpt:
            stop_audio_token = 1025
            last_latents = None

            @staticmethod
            def generate(cond, codes, **kw):
                calls["gen"].append(kw)
                M.gpt.last_latents = torch.zeros(1, 3, D)
                return torch.tensor([[5, 6, 1025]])

    import genvc_amd.engine as E
    monkeypatch.setattr(E, "resample", lambda wav, a, b: (calls["resample"].append((a, b)), torch.zeros(1, wav.shape[1] * b // a))[1])
    src = torch.zeros(1, 16000 * 2 + 100)
    IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, guidance_scale=1.5)
    assert len(calls["gen"]) == 3                                        # three segments
    assert calls["cond"] == [((1, 48150), 24000), ((1, 24000), 24000)]   # the negative (source, resampled) once, then the target
    assert calls["resample"] == [(16000, 24000)]
    negs = [kw["negative_cond_latents"] for kw in calls["gen"]]
    assert all(n is negs[0] for n in negs) and float(negs[0][0, 0, 0]) == 1.0
    assert all(kw["guidance_scale"] == 1.5 for kw in calls["gen"])
    # an explicit negative reference at the conditioning rate is not resampled
    for k in calls:
        calls[k].clear()
    IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, guidance_scale=1.5, negative_ref_audio=(torch.zeros(1, 30000), 24000))
    assert calls["resample"] == [] and calls["cond"][0] == ((1, 30000), 24000)
    # guidance off: nothing computed, nothing passed
    for off in (None, 1.0):
        for k in calls:
            calls[k].clear()
        IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, guidance_scale=off)
        assert len(calls["cond"]) == 1 and all("negative_cond_latents" not in kw for kw in calls["gen"])


def test_new_symbols_declared_and_exported():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s
