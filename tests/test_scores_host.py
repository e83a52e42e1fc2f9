"""CPU: return_dict_in_generate / output_scores / output_logits of GPT.generate: the kwarg handling and the result object on a
CPU-constructed GPT (the device loop replaced by a stand-in that fills the buffers it is given), the modes and paths that refuse the
kwargs by name, the new C ABI symbols, and tests/scores_oracle.py's gather against the installed transformers' own
GenerationMixin.compute_transition_scores, executed."""
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scores_oracle as SO                    # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gvc_gpt_generate_scores", "gvc_transition_scores")
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]
V, EOS = 1026, 1025
N_STEPS = 5          # the stand-in loop stops every row at this step


def cpu_gpt(max_slots=8):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"])
    g.max_slots = max_slots
    return g


def inputs(B=2, Tc=5):
    return torch.zeros(B, 32, D), torch.zeros(B, Tc, dtype=torch.long)


def stand_in(g, monkeypatch, max_new=9):
    """replaces the device side of generate(): _start hands out CPU loop state, _advance writes N_STEPS tokens (the last one the stop
    token) and marks every buffer it was given; -> the dict that records what _advance saw"""
    seen = {}

    def start(fake, kw, fan=1):
        B = int(fake.shape[0])
        return dict(B=B, ids=torch.zeros(B, 60, dtype=torch.int32), toks=torch.full((B, max_new), EOS, dtype=torch.int32),
                    lats=torch.zeros(B, max_new, D), max_new=max_new, done=0, n0=40, proc=None, warp=None)

    def advance(st, n):
        seen["scores"], seen["logits"], seen["do_sample"] = st.get("scores"), st.get("raw_logits"), st.get("do_sample")
        st["toks"][:, :N_STEPS - 1] = 7
        for key, base in (("scores", 100.0), ("raw_logits", 200.0)):
            if st.get(key) is not None:
                st[key][:] = base + torch.arange(max_new, dtype=torch.float32)[None, :, None]
        st["done"] = max_new
        return True

    monkeypatch.setattr(g, "compute_embeddings", lambda c, t: torch.ones(int(t.shape[0]), 40, dtype=torch.long))
    monkeypatch.setattr(g, "_start", start)
    monkeypatch.setattr(g, "_advance", advance)
    monkeypatch.setattr(g, "_recovering", lambda n, fn: fn())
    return seen


def test_return_dict_false_returns_the_tensor(monkeypatch):
    """absent or False: the bare tensor, whatever the other two say (HF ignores them then too), and no buffer is allocated"""
    g = cpu_gpt()
    seen = stand_in(g, monkeypatch)
    cond, codes = inputs()
    for kw in ({}, dict(return_dict_in_generate=False), dict(output_scores=True, output_logits=True),
               dict(return_dict_in_generate=False, output_scores=True), dict(return_dict_in_generate=None, output_logits=True)):
        out = g.generate(cond, codes, do_sample=False, **kw)
        assert torch.is_tensor(out) and out.dtype == torch.int64 and tuple(out.shape) == (2, N_STEPS)
        assert seen["scores"] is None and seen["logits"] is None


def test_result_object(monkeypatch):
    from genvc_amd.layers.gpt import GenerateOutput
    g = cpu_gpt()
    seen = stand_in(g, monkeypatch)
    cond, codes = inputs()
    plain = g.generate(cond, codes, do_sample=False)
    out = g.generate(cond, codes, do_sample=False, return_dict_in_generate=True)
    assert isinstance(out, GenerateOutput)
    assert torch.equal(out.sequences, plain) and out["sequences"] is out.sequences
    assert out.scores is None and out.logits is None and out.sequences_scores is None
    assert out.latents is g.last_latents and tuple(out.latents.shape) == (2, N_STEPS, D)
    assert seen["scores"] is None and seen["logits"] is None           # allocated only when asked for
    with pytest.raises(AttributeError):
        out.attentions
    with pytest.raises(KeyError):
        out["attentions"]
    for sc, lg in ((True, False), (False, True), (True, True)):
        out = g.generate(cond, codes, do_sample=False, return_dict_in_generate=True, output_scores=sc, output_logits=lg)
        assert torch.equal(out.sequences, plain)
        assert (seen["scores"] is not None) == sc and (seen["logits"] is not None) == lg and seen["do_sample"] is False
        for tup, on, buf, base in ((out.scores, sc, seen["scores"], 100.0), (out["logits"], lg, seen["logits"], 200.0)):
            if not on:
                assert tup is None
                continue
            # n views into the one [rows, max_new, V] tensor the loop filled, fp32
            assert isinstance(tup, tuple) and len(tup) == N_STEPS and tuple(buf.shape) == (2, 9, V) and buf.dtype == torch.float32
            for t, row in enumerate(tup):
                assert tuple(row.shape) == (2, V) and row.data_ptr() == buf[:, t].data_ptr() and bool((row == base + t).all())
    # sampling is HF's default
    g.generate(cond, codes, return_dict_in_generate=True, output_scores=True)
    assert seen["do_sample"] is True
    # num_return_sequences: rows = B * N
    monkeypatch.setattr(g, "sequence_logprobs", lambda t, l: (None, None))
    out = g.generate(cond, codes, num_return_sequences=3, return_dict_in_generate=True, output_scores=True)
    assert tuple(out.sequences.shape) == (6, N_STEPS) and tuple(out.scores[0].shape) == (6, V)


def test_modes_without_step_scores_refuse_by_name(monkeypatch):
    g = cpu_gpt(max_slots=16)
    cond, codes = inputs(B=1)
    rd = dict(return_dict_in_generate=True)
    with pytest.raises(NotImplementedError, match=r"output_scores=True with beam search \(num_beams=4\)"):
        g.generate(cond, codes, num_beams=4, do_sample=False, output_scores=True, **rd)
    with pytest.raises(NotImplementedError, match=r"output_logits=True with beam search \(num_beams=4\)"):
        g.generate(cond, codes, num_beams=4, do_sample=False, output_logits=True, **rd)
    with pytest.raises(NotImplementedError, match=r"output_scores=True with beam groups"):
        g.generate(cond, codes, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, do_sample=False, output_scores=True, **rd)
    with pytest.raises(NotImplementedError, match=r"output_scores=True with contrastive search \(penalty_alpha=0\.6\)"):
        g.generate(cond, codes, do_sample=False, top_k=4, penalty_alpha=0.6, output_scores=True, **rd)
    # return_dict_in_generate alone is served there, and so is output_scores without it (ignored)
    ids = torch.tensor([[3, 4, EOS]])
    g.last_latents = None
    for mode, kw in (("_generate_beams", dict(num_beams=4, do_sample=False)),
                     ("_generate_contrastive", dict(do_sample=False, top_k=4, penalty_alpha=0.6))):
        monkeypatch.setattr(g, mode, lambda c, t, k: (setattr(g, "last_beam_scores", torch.tensor([-1.5])), ids)[1])
        out = g.generate(cond, codes, **kw, **rd)
        assert out.sequences is ids and out.scores is None and out.logits is None
        assert (out.sequences_scores is g.last_beam_scores) == (mode == "_generate_beams")
        assert mode == "_generate_beams" or out.sequences_scores is None
        assert g.generate(cond, codes, output_scores=True, **kw) is ids


@pytest.mark.parametrize("key", ["return_dict_in_generate", "output_scores", "output_logits"])
def test_refused_paths_name_themselves(key):
    from genvc_amd.streaming import StreamSessions
    g = cpu_gpt()
    cond, codes = inputs(B=1)
    kw = {key: True}
    with pytest.raises(NotImplementedError, match=re.escape(f"{key}=True is not on the streaming (get_generator) path")):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))
    with pytest.raises(NotImplementedError, match=re.escape(f"{key}=True is not on the grouped (generate_groups) path")):
        g.generate_groups([(cond, codes)], **kw)
    with pytest.raises(NotImplementedError, match=re.escape(f"{key}=True is not on the rolling (generate_rolling) path")):
        g.generate_rolling([(cond, codes)], top_k=1, **kw)
    with pytest.raises(NotImplementedError, match=re.escape(f"{key}=True is not on the session (StreamSessions, open) path")):
        StreamSessions._procs(object(), dict(kw), {}, "open")
    # falsy: these paths behave as before (they reach the engine check); output_attentions / output_hidden_states keep their treatment
    for off in ({key: False}, {key: None}, dict(output_attentions=False, output_hidden_states=False)):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **off))
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate_groups([(cond, codes)], **off)
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate_rolling([(cond, codes)], top_k=1, **off)


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
    # the entry points that were there keep their signatures (a C ABI)
    assert len(_lib._SIGNATURES["gvc_gpt_generate_cfg"][1]) == 23 and len(_lib._SIGNATURES["gvc_gpt_generate_warp"][1]) == 21
    assert len(_lib._SIGNATURES["gvc_gpt_generate_scores"][1]) == 27


def rows_with_inf(R, n, seed):
    """scores [n][R, V] with -inf entries as the processors and warpers leave them: a banned handful in some rows, all but a
    top 15 in others; and tokens [R, n] that survive"""
    gen = torch.Generator().manual_seed(seed)
    scores, toks = [], []
    for t in range(n):
        s = (torch.rand(R, V, generator=gen) * 2 - 1) * 12.0
        for r in range(R):
            if (r + t) % 2 == 0:
                s[r, torch.randperm(V, generator=gen)[:7]] = -float("inf")
            else:
                s[r, s[r] < torch.topk(s[r], 15)[0][-1]] = -float("inf")
        keep = [torch.nonzero(torch.isfinite(s[r])).squeeze(1) for r in range(R)]
        toks.append(torch.stack([k[int(torch.randint(len(k), (1,), generator=gen))] for k in keep]))
        scores.append(s)
    return scores, torch.stack(toks, 1)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("R,n", [(1, 1), (3, 12)])
def test_oracle_gather_equals_the_executed_hf_method(R, n, normalize):
    scores, toks = rows_with_inf(R, n, 5 + R)
    assert any(bool(torch.isinf(s).any()) for s in scores)
    want = SO.hf_gather(scores, toks, normalize, V)
    got = SO.gather(scores, toks, normalize)
    assert tuple(want.shape) == (R, n) and torch.isfinite(want).all()
    assert torch.equal(got, want)
    # a prompt in front of the tokens is cut away, as HF cuts it
    assert torch.equal(SO.hf_gather(scores, torch.cat([torch.zeros(R, 4, dtype=torch.long), toks], 1), normalize, V), want)


def _infer(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--device", "cpu", *flags], capture_output=True, text=True,
                          env=env, cwd=ROOT)


def test_infer_token_scores_flag():
    r = _infer("--streaming", "--token_scores", "x.npz")
    assert r.returncode != 0 and "--token_scores is not on the streaming path (--streaming)" in r.stderr
    r = _infer("--token_scores", "x.npz", "--num_beams", "4")
    assert r.returncode != 0 and "--token_scores does not combine" in r.stderr


def test_harness_collects_token_logprobs():
    """synthesize_utt(token_scores=True): every segment's call asks for the scores and the details carry one log-prob row per segment,
    stop tokens dropped with the codes; without it the call is the one it was"""
    from genvc_amd.inference import inference_utils as IU
    from genvc_amd.layers.gpt import GenerateOutput
    calls = []

    class M:
        device = "cpu"
        content_sample_rate = 16000
        hifigan = None
        config = type("C", (), dict(audio=type("A", (), dict(sample_rate=24000))(), top_p=0.85, top_k=15, temperature=0.75,
                                    length_penalty=1.0, repetition_penalty=10.0,
                                    model_args=type("MA", (), dict(gpt_code_stride_len=1024))()))()

        def get_gpt_cond_latents(self, audio, sr):
            return torch.zeros(1, 32, D)

        class content_extractor:
            @staticmethod
            def extract_content_features(seg):
                return torch.zeros(1, 4, 8)

        class content_dvae:
            @staticmethod
            def get_codebook_indices(feat):
                return torch.zeros(1, 4, dtype=torch.long)

        class gpt:
            stop_audio_token = EOS
            last_latents = None

            @staticmethod
            def generate(cond, codes, **kw):
                calls.append(kw)
                M.gpt.last_latents = torch.zeros(1, 3, D)
                ids = torch.tensor([[5, 6, EOS]])
                if not kw.get("return_dict_in_generate"):
                    return ids
                return GenerateOutput(sequences=ids, scores=tuple(torch.zeros(1, V) for _ in range(3)), logits=None, latents=None,
                                      sequences_scores=None)

            @staticmethod
            def compute_transition_scores(sequences, scores, normalize_logits=False):
                assert normalize_logits and len(scores) == sequences.shape[1]
                return torch.tensor([[-0.5, -1.5, -2.5]])

    src = torch.zeros(1, 16000 * 2 + 100)
    out = IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, return_details=True, token_scores=True)
    assert len(calls) == 3 and all(kw["return_dict_in_generate"] and kw["output_scores"] for kw in calls)
    assert len(out["token_logprobs"]) == len(out["codes"]) == 3
    assert all(torch.equal(lp, torch.tensor([-0.5, -1.5])) for lp in out["token_logprobs"])
    calls.clear()
    out = IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, return_details=True)
    assert "token_logprobs" not in out and all("return_dict_in_generate" not in kw for kw in calls)
    with pytest.raises(ValueError, match="return_details"):
        IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, token_scores=True)
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, return_details=True, token_scores=True, num_return_sequences=2)
