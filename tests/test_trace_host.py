"""CPU: output_attentions / output_hidden_states of GPT.generate, GPT.trace and the alignment options: tests/trace_oracle.py against
every tests/golden/trace_*.npz (the reference's GPT2InferenceModel driven step by step, scripts/make_trace_golden.py), the kwarg
handling and the per-step views on a CPU-constructed GPT with a stub engine, the modes and paths that refuse the kwargs by name, the
size guard, the new C ABI symbol and the infer.py flag."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import act_stats                              # noqa: E402
import test_scores_host as SH                 # noqa: E402
import trace_oracle as TO                     # noqa: E402

ROOT = SH.ROOT
D, EOS, N_STEPS = SH.D, SH.EOS, SH.N_STEPS
L, H = 2, 4                   # gcfg.TINY_MODEL_ARGS
P = 39                        # prefix rows of the stand-in: 32 conditioning rows, text start, 5 content codes, text stop
ASK = dict(return_dict_in_generate=True, output_attentions=True, output_hidden_states=True)


# ---- the oracle against the reference's per-step outputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(TO.CASES))
def test_oracle_reproduces_the_reference_steps(tag, gold):
    """one teacher-forced pass of the oracle over the fixture's ids reproduces every step of the reference's cached loop: in float64
    within the stored floor (the reference's own fp32-versus-fp64 deviation), in float32 within the project's 8 floors"""
    f = gold(f"trace_{tag}")
    sh, dims = TO.SHAPES[tag], TO.case_dims(tag)
    n, nl = sh["steps"], dims["n_layer"]
    seed, bias = int(f["seed"]), float(f["stop_bias"])
    w = TO.case_weights(tag, seed, None if bias < 0 else bias)
    cond, codes = TO.case_inputs(tag, seed)
    ids = torch.from_numpy(f["tokens"])
    lengths = torch.from_numpy(f["lengths"])
    assert lengths.tolist() == TO.lengths_of(ids, dims["stop_audio_token"]).tolist()
    assert float(f["margins"][np.arange(n)[None, :] < f["lengths"][:, None]].min()) >= TO.MIN_MARGIN
    peak = TO.stored_peak_median([[f[f"att_{i}"][l] for l in range(nl)] for i in range(n)], lengths)
    assert min(peak) >= TO.MIN_PEAK and np.allclose(peak, f["peak"])
    Pp, cs = TO.N_COND + sh["Tc"] + 2, int(f["channel_step"])
    fa, fh = float(f["floor_att"]), float(f["floor_hid"])
    for name, ww, cc, margin in (("float64", act_stats.double(w), cond.double(), 1.0), ("float32", w, cond, 8.0)):
        att, hid = TO.steps_of(*TO.trace(ww, dims, cc, codes, ids), Pp, n)
        ea = eh = 0.0
        for i in range(n):
            live = lengths > i
            a, h = torch.stack(att[i]).double(), torch.stack(hid[i])[..., ::cs].double()
            ra, rh = torch.from_numpy(f[f"att_{i}"]).double(), torch.from_numpy(f[f"hid_{i}"]).double()
            assert a.shape == ra.shape and h.shape == rh.shape
            ea, eh = max(ea, float((a - ra)[:, live].abs().max())), max(eh, float((h - rh)[:, live].abs().max()))
        print(f"trace_{tag} {name}: attentions {ea:.3e} = {ea / fa:.2f} floors, hidden states {eh:.3e} = {eh / fh:.2f} floors")
        assert ea <= margin * fa * (1 + 1e-6) and eh <= margin * fh * (1 + 1e-6)


def test_fixture_files_are_small():
    for tag in TO.CASES:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"trace_{tag}.npz")) < 900 * 1024


# ---- kwarg handling on a CPU GPT with a stub engine ---------------------------------------------------------------------------------
class StubEngine:
    """stands in for GptEngine.trace: fills the full tensors with their own flat index, so a view's content names its place"""
    weight_dtype = "fp32"

    def __init__(self):
        self.calls = []

    def trace(self, slots, prefix, ids, lengths, n_cond, output_attentions=True, output_hidden_states=False, alignment=True,
              alignment_layers=None):
        B, Pn = int(prefix.shape[0]), int(prefix.shape[1])
        n = int(ids.shape[1])
        T = Pn + n
        self.calls.append(dict(slots=slots, prefix=prefix, ids=ids.clone(), lengths=torch.as_tensor(lengths).clone(), n_cond=n_cond,
                               alignment=alignment))
        probs = torch.arange(L * B * H * T * T, dtype=torch.float32).view(L, B, H, T, T) if output_attentions else None
        hidden = torch.arange((L + 1) * B * T * D, dtype=torch.float32).view(L + 1, B, T, D) if output_hidden_states else None
        return probs, hidden, None


def stand_in(g, monkeypatch):
    seen = SH.stand_in(g, monkeypatch)
    start0 = g._start

    def start(fake, kw, fan=1):
        st = start0(fake, kw, fan)
        st["slots"] = torch.arange(int(fake.shape[0]), dtype=torch.int32)
        return st

    def embed(c, t):
        g._prefix, g._n_cond = torch.zeros(int(t.shape[0]), P, D), int(c.shape[1])
        return torch.ones(int(t.shape[0]), P + 1, dtype=torch.long)
    monkeypatch.setattr(g, "_start", start)
    monkeypatch.setattr(g, "compute_embeddings", embed)
    g.engine = StubEngine()
    return seen


def test_kwargs_ignored_without_return_dict(monkeypatch):
    g = SH.cpu_gpt()
    stand_in(g, monkeypatch)
    cond, codes = SH.inputs()
    plain = g.generate(cond, codes, do_sample=False)
    for kw in (dict(output_attentions=True), dict(output_hidden_states=True), dict(return_dict_in_generate=False, **{k: True for k in
               ("output_attentions", "output_hidden_states")})):
        out = g.generate(cond, codes, do_sample=False, **kw)
        assert torch.is_tensor(out) and torch.equal(out, plain)
    assert g.engine.calls == []
    out = g.generate(cond, codes, do_sample=False, return_dict_in_generate=True, output_scores=True)
    assert g.engine.calls == [] and "attentions" not in out and "hidden_states" not in out


def test_step_views_shapes_and_strides(monkeypatch):
    from genvc_amd.layers.gpt import GenerateOutput
    g = SH.cpu_gpt()
    stand_in(g, monkeypatch)
    cond, codes = SH.inputs()
    plain = g.generate(cond, codes, do_sample=False)
    n, T = N_STEPS, P + N_STEPS
    for at, hs in ((True, True), (True, False), (False, True)):
        g.engine.calls.clear()
        out = g.generate(cond, codes, do_sample=False, return_dict_in_generate=True, output_attentions=at, output_hidden_states=hs)
        assert isinstance(out, GenerateOutput) and torch.equal(out.sequences, plain)
        (call,) = g.engine.calls                                            # one pass, after the tokens are final
        assert torch.equal(call["ids"].long(), plain) and call["ids"].dtype == torch.int32 and call["n_cond"] == 32
        assert call["lengths"].tolist() == [N_STEPS, N_STEPS] and call["alignment"] is False and tuple(call["prefix"].shape) == (2, P, D)
        assert (out.attentions is not None) == at and (out.hidden_states is not None) == hs
        if at:
            assert isinstance(out.attentions, tuple) and len(out.attentions) == n and all(len(s) == L for s in out.attentions)
            for i, step in enumerate(out.attentions):
                for l, v in enumerate(step):
                    rows, lo = (P + 1, 0) if i == 0 else (1, P + i)
                    assert tuple(v.shape) == (2, H, rows, P + 1 + i) and v.dtype == torch.float32
                    assert v.stride() == (H * T * T, T * T, T, 1)                 # a view into the one [L, rows, H, T, T] tensor
                    assert float(v[0, 0, 0, 0]) == float(l * 2 * H * T * T + lo * T) and float(v[1, 2, -1, -1]) == float(
                        ((l * 2 + 1) * H + 2) * T * T + (P + i) * T + P + i)
        if hs:
            assert len(out.hidden_states) == n and all(len(s) == L + 1 for s in out.hidden_states)
            for i, step in enumerate(out.hidden_states):
                for l, v in enumerate(step):
                    rows, lo = (P + 1, 0) if i == 0 else (1, P + i)
                    assert tuple(v.shape) == (2, rows, D) and v.stride() == (T * D, D, 1)
                    assert float(v[1, 0, 0]) == float(((l * 2 + 1) * T + lo) * D)
    # num_return_sequences: rows = B * N, the prefix of item b repeated for its candidates
    monkeypatch.setattr(g, "sequence_logprobs", lambda t, l: (None, None))
    g.engine.calls.clear()
    out = g.generate(cond, codes, num_return_sequences=3, **ASK)
    assert tuple(out.attentions[0][0].shape) == (6, H, P + 1, P + 1) and tuple(g.engine.calls[0]["prefix"].shape) == (6, P, D)


def test_size_guard(monkeypatch):
    g = SH.cpu_gpt()
    stand_in(g, monkeypatch)
    cond, codes = SH.inputs()
    T = P + N_STEPS
    size = 4 * L * 2 * H * T * T
    out = g.generate(cond, codes, do_sample=False, max_trace_bytes=size, **ASK)            # exactly the limit: served
    assert out.attentions is not None
    with pytest.raises(ValueError, match=rf"{size} bytes .*max_trace_bytes={size - 1}.*GPT\.trace\(\.\.\., output_attentions=False\)"):
        g.generate(cond, codes, do_sample=False, max_trace_bytes=size - 1, **ASK)
    # hidden states alone are not guarded; the default is 2 GiB
    assert g.generate(cond, codes, do_sample=False, max_trace_bytes=1, return_dict_in_generate=True, output_hidden_states=True).attentions is None
    from genvc_amd.layers import gpt as G
    assert G.MAX_TRACE_BYTES == 2 << 30
    with pytest.raises(ValueError, match="max_trace_bytes"):
        G._trace_bytes_check(30, 5, 16, 700, G.MAX_TRACE_BYTES)
    G._trace_bytes_check(30, 1, 16, 700, G.MAX_TRACE_BYTES)


def test_bf16_context_refuses_by_name(monkeypatch):
    g = SH.cpu_gpt()
    stand_in(g, monkeypatch)
    g.engine.weight_dtype = "bf16_mfma"
    cond, codes = SH.inputs()
    with pytest.raises(NotImplementedError, match='weight_dtype="bf16_mfma"'):
        g.generate(cond, codes, do_sample=False, **ASK)
    assert torch.is_tensor(g.generate(cond, codes, do_sample=False, output_attentions=True))       # ignored without the result object
    with pytest.raises(NotImplementedError, match='GPT.trace with weight_dtype="bf16_mfma"'):
        g.trace(cond, codes, torch.zeros(2, 4, dtype=torch.long))


@pytest.mark.parametrize("key", ["output_attentions", "output_hidden_states"])
def test_modes_refuse_by_name(key, monkeypatch):
    g = SH.cpu_gpt(max_slots=16)
    cond, codes = SH.inputs(B=1)
    kw = {"return_dict_in_generate": True, key: True}
    with pytest.raises(NotImplementedError, match=rf"{key}=True with beam search \(num_beams=4\)"):
        g.generate(cond, codes, num_beams=4, do_sample=False, **kw)
    with pytest.raises(NotImplementedError, match=rf"{key}=True with beam groups"):
        g.generate(cond, codes, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, do_sample=False, **kw)
    with pytest.raises(NotImplementedError, match=rf"{key}=True with contrastive search \(penalty_alpha=0\.6\)"):
        g.generate(cond, codes, do_sample=False, top_k=4, penalty_alpha=0.6, **kw)
    with pytest.raises(NotImplementedError, match=rf"{key}=True with assisted decoding \(assistant_model\)"):
        g.generate(cond, codes, do_sample=False, assistant_model=SH.cpu_gpt(), **kw)
    with pytest.raises(NotImplementedError, match=rf"{key}=True with prompt-lookup decoding \(prompt_lookup_num_tokens\)"):
        g.generate(cond, codes, do_sample=False, prompt_lookup_num_tokens=3, **kw)
    # without return_dict_in_generate the kwarg is ignored there too: the modes run as they always have
    ids = torch.tensor([[3, 4, EOS]])
    g.last_latents = None
    monkeypatch.setattr(g, "_generate_beams", lambda c, t, k: (setattr(g, "last_beam_scores", torch.tensor([-1.5])), ids)[1])
    assert g.generate(cond, codes, num_beams=4, do_sample=False, **{key: True}) is ids


def test_paths_refuse_by_name():
    """output_attentions=True names the path it is refused on.  output_hidden_states=True alone stays what it was there -- the reference's
    streaming harness passes it to get_generator to ask for the latents, which these paths yield anyway -- and as a request for a
    result object it is refused with return_dict_in_generate, by the path's name"""
    from genvc_amd.streaming import StreamSessions
    g = SH.cpu_gpt()
    cond, codes = SH.inputs(B=1)
    for kw, key in ((dict(output_attentions=True), "output_attentions"),
                    (dict(return_dict_in_generate=True, output_hidden_states=True), "return_dict_in_generate"),
                    (dict(return_dict_in_generate=True, output_attentions=True), "return_dict_in_generate")):
        with pytest.raises(NotImplementedError, match=re.escape(f"{key}=True is not on the streaming (get_generator) path")):
            next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))
        with pytest.raises(NotImplementedError, match=re.escape(f"{key}=True is not on the grouped (generate_groups) path")):
            g.generate_groups([(cond, codes)], **kw)
        with pytest.raises(NotImplementedError, match=re.escape(f"{key}=True is not on the rolling (generate_rolling) path")):
            g.generate_rolling([(cond, codes)], top_k=1, **kw)
        with pytest.raises(NotImplementedError, match=re.escape(f"{key}=True is not on the session (StreamSessions, open) path")):
            StreamSessions._procs(object(), dict(kw), {}, "open")
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):          # the harness' own spelling reaches the engine check
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), output_attentions=False, output_hidden_states=True))


def test_forward_return_attentions_points_to_trace():
    g = SH.cpu_gpt()
    g.engine = object()
    z = torch.zeros(1, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match=r"do not keep their weights.*GPT\.trace"):
        g.forward(z, torch.tensor([4]), z, torch.tensor([4096]), cond_latents=torch.zeros(1, 32, D), return_attentions=True)


# ---- the C ABI, the harness and the CLI ---------------------------------------------------------------------------------------------
def test_new_symbol_declared_and_exported():
    import ctypes as C
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    assert re.search(r"\bgvc_gpt_trace\(", hdr) and "typedef struct gvc_trace_options" in hdr
    assert "gvc_gpt_trace" in _lib.exported_symbols() and len(_lib._SIGNATURES["gvc_gpt_trace"][1]) == 11
    # the struct the binding fills is the header's: four int32, one uint64, four pointers
    fields = re.search(r"typedef struct gvc_trace_options \{(.*?)\} gvc_trace_options;", hdr, re.S).group(1)
    names = [n.strip() for decl in re.sub(r"/\*.*?\*/", "", fields, flags=re.S).split(";") if decl.strip()
             for n in decl.replace("*", " ").split(None, 1)[1].split(",")]
    assert names == [n for n, _ in _lib.TraceOptions._fields_]
    assert C.sizeof(_lib.TraceOptions) == 4 * 4 + 8 + 4 * C.sizeof(C.c_void_p)
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert "gvc_gpt_trace" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    # the entry points that were there keep their signatures
    assert len(_lib._SIGNATURES["gvc_gpt_latents"][1]) == 11 and len(_lib._SIGNATURES["gvc_gpt_forward_rows"][1]) == 12


def test_infer_alignment_flag():
    r = SH._infer("--streaming", "--alignment", "x.npz")
    assert r.returncode != 0 and "--alignment is not on the streaming path (--streaming)" in r.stderr
    r = SH._infer("--alignment", "x.npz", "--num_return_sequences", "2")
    assert r.returncode != 0 and "--alignment does not combine with --num_return_sequences" in r.stderr
    r = SH._infer("--alignment", "x.npz", "--weights", "bf16")
    assert r.returncode != 0 and "--alignment needs --weights fp32" in r.stderr
    r = SH._infer("--help")
    assert r.returncode == 0 and "--alignment PATH.npz" in r.stdout


def test_harness_collects_alignments():
    """synthesize_utt(alignment=True): one GPT.trace call per segment on the stop-free codes, one [n, Tc] matrix per segment in the
    details; GenVCModel.inference(return_alignment=True) returns the matrix beside the waveform"""
    from genvc_amd.inference import inference_utils as IU
    from genvc_amd.inference.model_init import GenVCModel
    from genvc_amd.layers.gpt import GenerateOutput
    traced = []

    class Gpt:
        stop_audio_token = EOS
        last_latents = None

        def generate(self, cond, codes, **kw):
            self.last_latents = torch.zeros(1, 3, D)
            return torch.tensor([[5, 6, EOS]])

        def trace(self, cond, codes, ids, output_attentions=True, **kw):
            traced.append((ids.clone(), output_attentions))
            return GenerateOutput(alignment=torch.full((1, ids.shape[1], codes.shape[1]), 0.125))

    class M:
        device = "cpu"
        content_sample_rate = 16000
        hifigan = None
        hifigan_scale_factor = 4
        config = type("C", (), dict(audio=type("A", (), dict(sample_rate=24000))(), top_p=0.85, top_k=15, temperature=0.75,
                                    length_penalty=1.0, repetition_penalty=10.0,
                                    model_args=type("MA", (), dict(gpt_code_stride_len=1024))()))()
        gpt = Gpt()

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

        _vocode_segment = lambda self, *a, **k: torch.zeros(1, 1, 2048)

    src = torch.zeros(1, 16000 * 2 + 100)
    out = IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, return_details=True, alignment=True)
    assert len(out["alignments"]) == len(out["codes"]) == 3 and all(tuple(a.shape) == (2, 4) for a in out["alignments"])
    assert len(traced) == 3 and all(ids.tolist() == [[5, 6]] and at is False for ids, at in traced)
    assert "alignments" not in IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, return_details=True)
    with pytest.raises(ValueError, match="return_details"):
        IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, alignment=True)
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        IU.synthesize_utt(M(), src, torch.zeros(1, 24000), seg_len=1.0, return_details=True, alignment=True, num_return_sequences=2)
    traced.clear()
    wav, al = GenVCModel.inference(M(), torch.zeros(1, 16000), torch.zeros(1, 32, D), return_alignment=True)
    assert tuple(wav.shape) == (1, 1, 2048) and tuple(al.shape) == (2, 4) and traced[0][0].tolist() == [[5, 6]]
    assert torch.is_tensor(GenVCModel.inference(M(), torch.zeros(1, 16000), torch.zeros(1, 32, D)))
    with pytest.raises(NotImplementedError, match="return_alignment=True with num_return_sequences"):
        GenVCModel.inference(M(), torch.zeros(1, 16000), torch.zeros(1, 32, D), return_alignment=True, num_return_sequences=2)
