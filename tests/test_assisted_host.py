"""CPU: assisted decoding (GPT.generate(assistant_model=...)): the validation of the kwargs on CPU-constructed GPTs, the modes and paths
that refuse it by name, the host loop driven through an engine stand-in, the unchanged call without an assistant, the numpy
restatement of the accept step against the plain greedy loop it must reproduce, and the new C ABI symbols."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assist_oracle as AO                    # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gvc_gpt_verify", "gvc_gpt_truncate", "gvc_spec_accept", "gvc_gpt_generate_assisted")
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]
MODE = re.escape("assisted decoding (assistant_model)")


def cpu_gpt(max_slots=8, **more):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(**dict(dict(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"]), **more))
    g.max_slots = max_slots
    return g


def inputs(B=2, Tc=5):
    return torch.zeros(B, 32, D), torch.zeros(B, Tc, dtype=torch.long)


def ready(g):
    """an `engine` that is not None: the checks that come before any device work see an initialised model"""
    g.engine = type("E", (), dict(dims=g.dims()))()
    return g


def test_assistant_must_be_an_initialised_matching_gpt():
    g = cpu_gpt()
    cond, codes = inputs()
    kw = dict(do_sample=False)
    with pytest.raises(ValueError, match=MODE + ": the assistant is not initialised"):
        g.generate(cond, codes, assistant_model=cpu_gpt(), **kw)
    with pytest.raises(ValueError, match=MODE + ": assistant_model must be another GPT"):
        g.generate(cond, codes, assistant_model=g, **kw)
    with pytest.raises(ValueError, match=MODE + ": assistant_model must be another GPT"):
        g.generate(cond, codes, assistant_model=object(), **kw)
    with pytest.raises(ValueError, match=MODE + ": the assistant's num_audio_tokens is 514"):
        g.generate(cond, codes, assistant_model=ready(cpu_gpt(num_audio_tokens=514, start_audio_token=512, stop_audio_token=513)), **kw)
    with pytest.raises(ValueError, match=MODE + ": the assistant's stop_audio_token is 1023"):
        g.generate(cond, codes, assistant_model=ready(cpu_gpt(stop_audio_token=1023)), **kw)
    with pytest.raises(ValueError, match=MODE + ": the assistant's start_audio_token is 1022"):
        g.generate(cond, codes, assistant_model=ready(cpu_gpt(start_audio_token=1022)), **kw)
    with pytest.raises(ValueError, match=MODE + ": assistant_cond_latents is required"):
        g.generate(cond, codes, assistant_model=ready(cpu_gpt(model_dim=512)), **kw)
    with pytest.raises(ValueError, match=MODE + r": 2 items need 2 KV slots in both contexts"):
        g.generate(cond, codes, assistant_model=ready(cpu_gpt(max_slots=1)), **kw)
    # a valid call gets as far as the target's engine check (no engine on this CPU-only module)
    for more in ({}, dict(num_assistant_tokens=1), dict(num_assistant_tokens=15), dict(num_assistant_tokens_schedule="constant"),
                 dict(do_sample=True, top_k=1), dict(repetition_penalty=2.0, no_repeat_ngram_size=2, min_new_tokens=3)):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate(cond, codes, assistant_model=ready(cpu_gpt()), **dict(kw, **more))
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
        g.generate(cond, codes, assistant_model=ready(cpu_gpt(model_dim=512)), assistant_cond_latents=torch.zeros(2, 32, 512), **kw)


@pytest.mark.parametrize("k", [0, 16, -1, 2.0, True, "5"])
def test_num_assistant_tokens_out_of_range(k):
    g = cpu_gpt()
    cond, codes = inputs()
    with pytest.raises(ValueError, match=r"num_assistant_tokens must be an int in \[1, 15\] for " + MODE):
        g.generate(cond, codes, assistant_model=ready(cpu_gpt()), do_sample=False, num_assistant_tokens=k)


def test_rows_and_schedule():
    g = cpu_gpt(max_slots=64)
    cond, codes = inputs(B=9)
    with pytest.raises(ValueError, match=MODE + r": 9 items x \(num_assistant_tokens \+ 1 = 16\) rows exceed the 128 rows"):
        g.generate(cond, codes, assistant_model=ready(cpu_gpt(max_slots=64)), do_sample=False, num_assistant_tokens=15)
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):          # 8 x 16 = 128 rows fit
        g.generate(*inputs(B=8), assistant_model=ready(cpu_gpt(max_slots=64)), do_sample=False, num_assistant_tokens=15)
    for sched in ("heuristic", "heuristic_transient"):
        with pytest.raises(ValueError, match=f"num_assistant_tokens_schedule='{sched}' with " + MODE):
            g.generate(*inputs(), assistant_model=ready(cpu_gpt()), do_sample=False, num_assistant_tokens_schedule=sched)


def test_combinations_raise_by_name():
    g = cpu_gpt(max_slots=16)
    cond, codes = inputs(B=1)
    a = ready(cpu_gpt())
    cases = [(dict(), r"sampling \(do_sample=True, top_k=0\) with " + MODE),
             (dict(do_sample=True, top_k=15), r"sampling \(do_sample=True, top_k=15\) with " + MODE),
             (dict(do_sample=False, num_beams=4), r"beam search \(num_beams=4\) with " + MODE),
             (dict(do_sample=False, num_beams=4, num_beam_groups=2, diversity_penalty=0.5), "beam groups .* with " + MODE),
             (dict(do_sample=False, top_k=4, penalty_alpha=0.6), r"contrastive search \(penalty_alpha=0.6\) with " + MODE),
             (dict(do_sample=False, guidance_scale=2.0, negative_cond_latents=cond), r"guidance_scale=2.0 with " + MODE),
             (dict(do_sample=False, num_return_sequences=3), "num_return_sequences=3 with " + MODE),
             (dict(do_sample=False, return_dict_in_generate=True, output_scores=True), "output_scores=True with " + MODE),
             (dict(do_sample=False, return_dict_in_generate=True, output_logits=True), "output_logits=True with " + MODE),
             (dict(do_sample=False, sequence_bias={(5,): 1.0}), "sequence_bias=.* is not served with " + MODE),
             (dict(do_sample=False, bad_words_ids=[[5]]), "bad_words_ids=.* is not served with " + MODE),
             (dict(do_sample=False, forced_eos_token_id=1025), "forced_eos_token_id=.* is not served with " + MODE),
             (dict(do_sample=False, renormalize_logits=True), "renormalize_logits=.* is not served with " + MODE)]
    for kw, msg in cases:
        with pytest.raises(NotImplementedError, match=msg):
            g.generate(cond, codes, assistant_model=a, **kw)


def test_refused_paths_name_themselves():
    from genvc_amd.inference.inference_utils import synthesize_utt_streaming
    from genvc_amd.streaming import StreamSessions
    g = cpu_gpt()
    cond, codes = inputs(B=1)
    kw = dict(assistant_model=ready(cpu_gpt()), do_sample=False)
    for where, call in (("streaming (get_generator)", lambda: next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))),
                        ("grouped (generate_groups)", lambda: g.generate_groups([(cond, codes)], **kw)),
                        ("rolling (generate_rolling)", lambda: g.generate_rolling([(cond, codes)], **kw)),
                        ("session (StreamSessions, open)", lambda: StreamSessions._procs(object(), dict(kw), {}, "open")),
                        ("streaming (synthesize_utt_streaming, infer.py --streaming)",
                         lambda: synthesize_utt_streaming(None, None, None, generate_kwargs=kw))):
        with pytest.raises(NotImplementedError, match=re.escape(f"assisted decoding (assistant_model) is not on the {where} path")):
            call()
    # assistant_model=None: these paths behave as before
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
        g.generate_groups([(cond, codes)], assistant_model=None)


@pytest.mark.parametrize("off", [dict(assistant_model=None), dict(assistant_model=None, num_assistant_tokens=3), {}])
def test_without_an_assistant_the_existing_path_is_unchanged(off, monkeypatch):
    """no assistant: the sampler loop gets the caller's kwargs as they are and makes exactly today's engine call"""
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
    monkeypatch.setattr(g, "_generate_assisted", lambda *a, **k: pytest.fail("assisted branch taken without an assistant"))
    kw = dict(do_sample=False, repetition_penalty=2.0, max_new_tokens=7, **off)
    with pytest.raises(Reached):
        g.generate(cond, codes, **kw)
    assert seen.pop("fan") == 1
    assert set(seen) == set(kw) and all(seen[k] is kw[k] for k in kw)


class StandIn:
    """an engine stand-in: records the calls of the plain loop, and plays the device's part of an assisted generation on the CPU (a
    fixed number of tokens per round and row)"""

    def __init__(self, g, per_round=(2, 4)):
        self.dims = g.dims()
        self.calls = []
        self.per_round = per_round

    def prefix_embeddings(self, cond, codes):
        return torch.zeros(cond.shape[0], cond.shape[1] + codes.shape[1] + 2, cond.shape[2])

    def prefill(self, slots, prefix, want_outputs=True, n_cached=0):
        self.calls.append(("prefill", tuple(slots.tolist()), tuple(prefix.shape), want_outputs, n_cached))

    def generate(self, slots, ids, ids_len, finished, params, i0, n_steps, toks, lats, max_keys=0, **kw):
        self.calls.append(("generate", i0, n_steps, max_keys, sorted(kw)))
        toks[:, i0:i0 + n_steps] = 7

    def generate_assisted(self, assistant, slots, aslots, st, params, n_rounds, max_keys, a_max_keys, proc=None, k=None):
        self.calls.append(("generate_assisted", n_rounds, k, max_keys, a_max_keys, proc is not None, params.top_k,
                           params.repetition_penalty))
        for b in range(st.B):
            if not st.opened:
                st.toks[b, 0] = 7
                st.emitted[b] = 1
            for _ in range(n_rounds):
                if st.finished[b]:
                    continue
                n = min(self.per_round[b % len(self.per_round)], k + 1, st.max_new - int(st.emitted[b]))
                st.toks[b, int(st.emitted[b]):int(st.emitted[b]) + n] = 7
                st.emitted[b] += n
                st.rounds[b] += 1
                st.finished[b] = int(st.emitted[b] >= st.max_new)
        st.opened = True

    def health(self):
        self.calls.append(("health",))

    def reset(self, slots):
        self.calls.append(("reset",))


def test_host_loop_through_a_stand_in():
    import genvc_amd.engine as E
    import genvc_amd.layers.gpt as G
    g, a = cpu_gpt(), cpu_gpt()
    g.engine, a.engine = StandIn(g), StandIn(a)
    cond, codes = inputs(B=2, Tc=5)
    n0 = 32 + 5 + 2 + 1
    out = g.generate(cond, codes, assistant_model=a, do_sample=False, repetition_penalty=2.0, num_assistant_tokens=3, max_new_tokens=12,
                     no_repeat_ngram_size=2, group=8)
    assert out.shape == (2, 12) and out.dtype == torch.int64 and bool((out == 7).all())
    assert g.last_latents.shape == (2, 12, D)
    assert set(g.last_assist_stats) == {"rounds", "drafted", "accepted"}
    assert all(t.dtype == torch.int64 and tuple(t.shape) == (2,) for t in g.last_assist_stats.values())
    calls = [c for c in g.engine.calls if c[0] == "generate_assisted"]
    # group 8 with k = 3: two rounds per host check; the slow row (2 tokens per round) needs 6 rounds for its 11 tokens
    assert [c[1] for c in calls] == [2, 2, 2] and all(c[2] == 3 for c in calls)
    assert all(c[5:] == (True, 1, 2.0) for c in calls)
    # cached positions a call can reach: the furthest row may have emitted 1 + rounds * (k + 1) tokens, at most max_new - 1
    assert [c[3] for c in calls] == [n0 + 5 + 3, n0 + 11 + 3, n0 + 11 + 3] and all(c[3] == c[4] for c in calls)
    assert g.engine.calls[0][:2] == ("prefill", (0, 1)) and a.engine.calls[0][:2] == ("prefill", (0, 1))
    assert g.engine.calls.count(("health",)) == 3 and a.engine.calls.count(("health",)) == 3
    assert not any(c[0] == "generate" for c in g.engine.calls)
    # the same GPT without the assistant: today's plain call, with today's arguments
    g.engine.calls.clear()
    out = g.generate(cond, codes, do_sample=False, repetition_penalty=2.0, max_new_tokens=12, no_repeat_ngram_size=2, group=8)
    assert [c for c in g.engine.calls if c[0] == "generate"] == [("generate", 0, 8, n0 + 8, ["proc"]), ("generate", 8, 4, n0 + 12, ["proc"])]
    assert not any(c[0] == "generate_assisted" for c in g.engine.calls)
    assert E.MAX_ASSISTANT_TOKENS == 15 and E.MAX_VERIFY_ROWS == 128 and "assistant_model" in G.ASSIST_KWARGS


def test_drafts_shrink_at_the_end_of_the_position_table():
    """the default budget (max_gen_mel_tokens) leaves 5 mel positions behind the last token: k = 7 drafts 7 until the furthest row could
    reach them, then 5"""
    g, a = cpu_gpt(max_mel_tokens=30), cpu_gpt(max_mel_tokens=30)
    g.engine, a.engine = StandIn(g, per_round=(8,)), StandIn(a)
    assert g.max_gen_mel_tokens == 27 and g.dims()["max_mel_pos"] == 33
    out = g.generate(*inputs(B=1), assistant_model=a, do_sample=False, num_assistant_tokens=7, group=1)
    assert out.shape == (1, 27)
    ks = [c[2] for c in g.engine.calls if c[0] == "generate_assisted"]
    # 33 - 2 - ub >= 7 while ub <= 24: rounds start at ub = 1, 9, 17 with 7 drafts, then at 25 with 33 - 2 - 25 = 6 ... the
    # stand-in emits min(8, k + 1) per round, so the fourth round is the last
    assert ks == [7, 7, 7, 6]
    with pytest.raises(ValueError, match="leaves no room for a draft"):
        g.generate(*inputs(B=1), assistant_model=a, do_sample=False, max_new_tokens=32)


def test_accept_restatement_reproduces_plain_greedy():
    """the numpy accept step (what the kernel is compared with on the GPU) driven over random per-position logits with random
    drafts: whatever is drafted, the emitted tokens are those of the plain greedy chain over the same logits"""
    rng = np.random.default_rng(3)
    V, EOS, n0, max_new, k, d = 64, 63, 5, 12, 3, 4
    # a "model" whose logits row depends on the position only
    table = rng.normal(size=(n0 + max_new + 1, V)).astype(np.float32)
    table[n0 + 9, EOS] = 50.0
    for rep, kw in ((1.0, {}), (2.0, {"no_repeat_ngram_size": 2}), (1.0, {"min_new_tokens": 11})):
        row, plain = [1] * n0, []
        while len(plain) < max_new:
            tok, _ = AO.chain_token(table[len(row)], row, n0, kw, rep, EOS)
            plain.append(tok)
            row.append(tok)
            if tok == EOS:
                break
        st = dict(ids=np.ones((1, n0 + max_new + 16), dtype=np.int32), ids_len=np.array([n0]), finished=np.zeros(1, dtype=np.int32),
                  emitted=np.zeros(1, dtype=np.int32), pending=np.full(1, -1), toks=np.full((1, max_new), EOS),
                  lats=np.zeros((1, max_new, d), dtype=np.float32), drop_target=np.zeros(1, dtype=np.int32),
                  drop_assistant=np.zeros(1, dtype=np.int32), rounds=np.zeros(1, dtype=np.int32), drafted=np.zeros(1, dtype=np.int32),
                  accepted=np.zeros(1, dtype=np.int32), max_new=max_new)
        AO.accept(st, 0, 0, table[None, n0:n0 + 1], np.zeros((1, 1, d), np.float32), None, rep, EOS, kw, n0)
        cached = n0          # positions in the "cache": everything but the pending token
        while not st["finished"][0]:
            good = plain[int(st["emitted"][0]):int(st["emitted"][0]) + k]
            drafts = np.array([[g if rng.random() < 0.6 else (g + 1) % (V - 1) for g in good] + [0] * (k - len(good))])
            pos = cached + 1 + np.arange(k + 1)          # row i is the model's output after [pending, d_1..d_i]
            AO.accept(st, k, k + 1, table[None, np.minimum(pos, len(table) - 1)], np.zeros((1, k + 1, d), np.float32), drafts, rep, EOS,
                      kw, n0)
            cached += k + 1 - int(st["drop_target"][0])
            assert cached == n0 + int(st["emitted"][0]) - 1
        n = int(st["emitted"][0])
        assert list(st["toks"][0, :n]) == plain[:n] and n == len(plain)
        assert st["accepted"][0] <= st["drafted"][0] <= k * st["rounds"][0]


def test_harness_passes_the_kwargs_through():
    """synthesize_utt hands generate_kwargs to every segment's generate call: assistant_model, num_assistant_tokens and
    assistant_cond_latents arrive as given, over the harness's own sampling kwargs"""
    from genvc_amd.inference import inference_utils as IU
    seen = []

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
            stop_audio_token = 1025
            last_latents = None

            @staticmethod
            def generate(cond, codes, **kw):
                seen.append(kw)
                M.gpt.last_latents = torch.zeros(1, 3, D)
                return torch.tensor([[5, 6, 1025]])

    draft, acond = object(), torch.zeros(1, 32, D)
    gkw = dict(assistant_model=draft, num_assistant_tokens=3, assistant_cond_latents=acond, do_sample=False)
    IU.synthesize_utt(M(), torch.zeros(1, 16000 * 2 + 100), torch.zeros(1, 24000), seg_len=1.0, generate_kwargs=gkw)
    assert len(seen) == 3
    for kw in seen:
        assert kw["assistant_model"] is draft and kw["assistant_cond_latents"] is acond and kw["num_assistant_tokens"] == 3
        assert kw["do_sample"] is False and kw["repetition_penalty"] == 10.0


def _infer(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--device", "cpu", *flags], capture_output=True, text=True,
                          env=env, cwd=ROOT)


def test_infer_flags():
    r = _infer("--assistant_layers", "2")
    assert r.returncode != 0 and "--assistant_layers needs --synthetic" in r.stderr
    r = _infer("--synthetic", "--streaming", "--assistant_layers", "2")
    assert r.returncode != 0 and "--assistant_layers is not on the streaming path (--streaming)" in r.stderr
    r = _infer("--synthetic", "--assistant_layers", "2", "--num_assistant_tokens", "3", "--num_beams", "4")
    assert r.returncode != 0 and "--assistant_layers decodes greedily" in r.stderr


def test_new_symbols_declared_and_exported():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    assert "gvc_spec_state" in hdr and _lib.SpecState._fields_[0][0] == "B"
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s
