"""CPU: the green-list watermark (watermarking_config; include/genvc_hip.h: gvc_logits_watermark, gvc_wm_score) -- the
host tables and the restatement tests/watermark_oracle.py pinned to the installed transformers EXECUTED with device="cpu"
(WatermarkLogitsProcessor, _get_logits_processor, WatermarkDetector), validation of the kwarg, the off spelling that passes no table,
the refusals by name, the infer.py and detect_watermark.py flags, the C ABI's struct and symbols."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ras_oracle as RO                    # noqa: E402
import watermark_oracle as WM              # noqa: E402
from genvc_amd import config as gcfg      # noqa: E402

V, EOS = 1026, 1025
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]
SYMBOLS = ("gvc_sample_wm", "gvc_gpt_generate_wm", "gvc_wm_score")
KEYS = (WM.DEFAULT_KEY, 2 ** 62 + 12345)          # the default, and one whose products with an id exceed 2**64
CFG = dict(greenlist_ratio=0.25, bias=2.0, hashing_key=WM.DEFAULT_KEY, seeding_scheme="lefthash", context_width=1)


def cpu_gpt(max_slots=16):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"])
    g.max_slots = max_slots
    return g


def hf_processor(vocab, key, ratio, scheme, bias=2.0):
    from transformers.generation.logits_process import WatermarkLogitsProcessor
    return WatermarkLogitsProcessor(vocab, "cpu", greenlist_ratio=ratio, bias=bias, hashing_key=key, seeding_scheme=scheme, context_width=1)


def unpack(table, vocab):
    """uint32 [rows, words] -> bool [rows, vocab]"""
    a = table.numpy().astype(np.uint32)
    bits = np.unpackbits(a.view(np.uint8).reshape(a.shape[0], -1), axis=1, bitorder="little")
    assert not bits[:, vocab:].any(), "a bit past the vocabulary is set"
    return bits[:, :vocab].astype(bool)


# ---- 1. the tables ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.25, 0.5])
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("vocab", [1026, 70])
def test_lefthash_table_is_the_installed_processors_greenlist_for_every_row(vocab, key, ratio):
    from genvc_amd.engine import WatermarkSettings, watermark_table
    t = watermark_table(WatermarkSettings(ratio, 2.0, key, "lefthash", 1), vocab)
    assert t.dtype == torch.uint32 and tuple(t.shape) == (vocab, (vocab + 31) // 32) and t.device.type == "cpu"
    got = unpack(t, vocab)
    hf = hf_processor(vocab, key, ratio, "lefthash")
    lists = WM.lefthash_lists(vocab, key, ratio)
    for prev in range(vocab):
        want = sorted(hf._get_greenlist_ids(torch.tensor([3, prev])).tolist())
        assert len(want) == int(vocab * ratio)
        assert np.flatnonzero(got[prev]).tolist() == want, prev
        assert sorted(lists[prev]) == want, prev
    assert watermark_table(WatermarkSettings(ratio, -1.0, key, "lefthash", 1), vocab) is t          # cached per (key, ratio, scheme, V)


@pytest.mark.parametrize("ratio", [0.25, 0.5])
@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("vocab", [1026, 70])
def test_selfhash_vector_is_membership_in_the_installed_processors_greenlist(vocab, key, ratio):
    from genvc_amd.engine import WatermarkSettings, watermark_table
    t = watermark_table(WatermarkSettings(ratio, 2.0, key, "selfhash", 1), vocab)
    assert t.dtype == torch.uint32 and tuple(t.shape) == (1, (vocab + 31) // 32)
    got = unpack(t, vocab)[0]
    hf = hf_processor(vocab, key, ratio, "selfhash")
    want = [c for c in range(vocab) if c in hf._get_greenlist_ids(torch.tensor([c])).tolist()]
    assert np.flatnonzero(got).tolist() == want
    assert sorted(WM.selfhash_set(vocab, key, ratio)) == want
    if (vocab, key, ratio) == (1026, WM.DEFAULT_KEY, 0.25):
        assert len(want) == 264


# ---- 2. the mark's place in the chain -----------------------------------------------------------------------------------------------
def test_installed_chain_puts_the_mark_behind_the_last_warper_and_ahead_of_normalisation():
    from transformers import GenerationConfig, GenerationMixin
    from transformers.generation.configuration_utils import WatermarkingConfig
    cfg = GenerationConfig(eos_token_id=EOS, pad_token_id=EOS, do_sample=True, temperature=0.8, top_k=15, top_p=0.9, min_p=0.05,
                           typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=1e-3, renormalize_logits=True, repetition_penalty=1.2,
                           min_new_tokens=3, watermarking_config=WatermarkingConfig(**CFG))
    cfg._eos_token_tensor = torch.tensor([EOS])

    class _M:
        config = type("C", (), {"is_encoder_decoder": False, "vocab_size": V, "get_text_config": lambda self, decoder=True: self})()
        _merge_criteria_processor_list = GenerationMixin._merge_criteria_processor_list
    names = [type(p).__name__ for p in GenerationMixin._get_logits_processor(_M(), generation_config=cfg, input_ids_seq_length=40,
                                                                             encoder_input_ids=None, logits_processor=None, device="cpu")]
    assert names[-2:] == ["WatermarkLogitsProcessor", "LogitNormalization"], names
    warpers = ["TemperatureLogitsWarper", "TopKLogitsWarper", "TopPLogitsWarper", "MinPLogitsWarper", "TypicalLogitsWarper",
               "EpsilonLogitsWarper", "EtaLogitsWarper"]
    assert all(w in names for w in warpers) and max(names.index(w) for w in warpers) == len(names) - 3, names


# ---- 3. the processor step ----------------------------------------------------------------------------------------------------------
def _logits(seed, vocab=V):
    return torch.randn(vocab, generator=torch.Generator().manual_seed(seed)) * 3.0


@pytest.mark.parametrize("scheme", ["lefthash", "selfhash"])
@pytest.mark.parametrize("samp", [dict(top_k=0, top_p=1.0), dict(top_k=15, top_p=1.0), dict(top_k=40, top_p=1.0), dict(top_k=0, top_p=0.9),
                                  dict(top_k=40, top_p=0.9)], ids=["k0", "k15", "k40", "p09", "k40_p09"])
def test_oracle_step_is_the_installed_processors_call_on_warped_rows(scheme, samp):
    wm = dict(key=WM.DEFAULT_KEY, ratio=0.25, scheme=scheme, bias=2.0)
    hf = hf_processor(V, wm["key"], wm["ratio"], scheme, wm["bias"])
    n = moved = 0
    for seed, prev in enumerate((0, 1, 5, 31, 32, 513, 1023, 1024, 1025)):
        s = RO.truncated_row(_logits(seed) / 0.8, dict(samp), {})
        if scheme == "selfhash" and WM.rank_tie(s):
            continue
        got = WM.mark_row(s, wm, prev)
        want = hf(torch.tensor([[7, prev]]), s[None].clone())[0]
        assert torch.equal(got, want), (seed, prev)
        moved += int(not torch.equal(got, s))          # (a row whose few survivors hold no green id stays as it is)
        n += 1
    assert n >= 6 and moved >= n - 2


def test_oracle_step_on_a_greedy_row_and_negative_and_zero_bias():
    for bias in (2.0, -1.5, 0.0):
        wm = dict(key=KEYS[1], ratio=0.5, scheme="lefthash", bias=bias)
        hf = hf_processor(V, wm["key"], wm["ratio"], "lefthash", bias)
        for seed, prev in enumerate((2, 1025, 40)):
            s = _logits(50 + seed)
            want = hf(torch.tensor([[prev]]), s[None].clone())[0]
            assert torch.equal(WM.mark_row(s, wm, prev), want)
            if bias == 0.0:
                assert torch.equal(want, s)
    # a previous id outside the vocabulary: no mark at this step
    assert torch.equal(WM.mark_row(_logits(3), dict(key=KEYS[0], ratio=0.25, scheme="lefthash", bias=2.0), -1), _logits(3))
    assert torch.equal(WM.mark_row(_logits(3), dict(key=KEYS[0], ratio=0.25, scheme="lefthash", bias=2.0), V), _logits(3))


def test_oracle_sampler_step_without_a_mark_is_the_plain_oracle():
    import penalty_oracle as PN
    samp = dict(repetition_penalty=1.3, temperature=0.8, top_p=0.85, top_k=15)
    row = [1, 1, 1024, 40, 41]
    a = WM.step(_logits(9), row, 3, samp, {}, None, (3, 5, 1), EOS)
    b = PN.step(_logits(9), row, 3, samp, {}, None, (3, 5, 1), EOS)
    assert (a["tok"], a["margin1"]) == (b["tok"], b["margin1"])


# ---- 4. the detector ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("scheme", ["lefthash", "selfhash"])
@pytest.mark.parametrize("n", [2, 3, 64, 600])
def test_oracle_detector_is_the_installed_detector(n, scheme, ignore):
    from transformers.generation.watermarking import WatermarkDetector
    from genvc_amd.engine import watermark_statistics
    vocab = 70          # (600 codes over 70 ids: repeated n-grams are certain)
    stub = type("Cfg", (), {"vocab_size": vocab, "bos_token_id": None, "is_encoder_decoder": False})()
    cfg = dict(CFG, seeding_scheme=scheme, hashing_key=KEYS[1], greenlist_ratio=0.5)
    hf = WatermarkDetector(stub, "cpu", cfg, ignore_repeated_ngrams=ignore)
    wm = dict(key=KEYS[1], ratio=0.5, scheme=scheme, bias=2.0)
    codes = torch.randint(0, vocab, (n,), generator=torch.Generator().manual_seed(n)).tolist()
    want = hf(torch.tensor([codes]), return_dict=True)
    scored, green, flags = WM.detector_flags(codes, n, vocab, wm, ignore_repeated=ignore)
    if ignore:
        # "counts a green/red hit once per unique ngram" (transformers' comment).  The installed _score_ngrams_in_passage builds its
        # Counter over TENSORS, which hash by identity, so it finds no two n-grams equal; the rule is executed here over n-grams as
        # tuples, every green decision being the installed detector's own _get_ngram_score, and the statistics its own formulas
        grams = {(c,) if scheme == "selfhash" else (p, c) for p, c in zip([None] + codes[:-1], codes) if scheme == "selfhash" or p is not None}
        hits = sum(int(hf._get_ngram_score(torch.tensor(g if scheme == "selfhash" else g[:-1]), torch.tensor(g[-1]))) for g in grams)
        cnt, grn = np.array([float(len(grams))]), np.array([float(hits)])
        zs = hf._compute_z_score(grn, cnt)
        want = type(want)(num_tokens_scored=cnt, num_green_tokens=grn, green_fraction=grn / cnt, z_score=zs, p_value=hf._compute_pval(zs),
                          prediction=zs > 3.0, confidence=1 - hf._compute_pval(zs))
        assert n < 600 or len(grams) < n - 1          # (the long sequence does repeat n-grams)
    assert (scored, green) == (int(want.num_tokens_scored[0]), int(want.num_green_tokens[0]))
    assert scored == sum(f != 2 for f in flags) and green == sum(f == 1 for f in flags)
    if not ignore:
        assert scored == (n - 1 if scheme == "lefthash" else n)
    z, p = WM.statistics(scored, green, 0.5)
    assert abs(z - float(want.z_score[0])) <= 1e-12 and abs(p - float(want.p_value[0])) <= 1e-12
    st = watermark_statistics(np.array([[scored, green]]), 0.5)
    assert abs(float(st["z_score"][0]) - float(want.z_score[0])) <= 1e-12 and abs(float(st["p_value"][0]) - float(want.p_value[0])) <= 1e-12
    assert bool(st["prediction"][0]) == bool(want.prediction[0]) and abs(float(st["confidence"][0]) - float(want.confidence[0])) <= 1e-12
    assert abs(float(st["green_fraction"][0]) - float(want.green_fraction[0])) <= 1e-12


def test_oracle_detector_skips_ids_outside_the_vocabulary_and_positions_past_the_length():
    wm = dict(key=KEYS[0], ratio=0.25, scheme="lefthash", bias=2.0)
    codes = [3, 4, 2000, 5, -1, 6, 7, 8]
    scored, _, flags = WM.detector_flags(codes, 7, V, wm)
    assert flags[0] == 2 and flags[2] == 2 and flags[3] == 2 and flags[4] == 2 and flags[5] == 2 and flags[7] == 2
    assert scored == 2 and flags[1] != 2 and flags[6] != 2
    scored, _, flags = WM.detector_flags(codes, 7, V, dict(wm, scheme="selfhash"))
    assert scored == 5 and flags[2] == 2 and flags[4] == 2 and flags[7] == 2


# ---- 5. the kwarg -------------------------------------------------------------------------------------------------------------------
def test_settings_defaults_dict_and_config_object():
    from transformers.generation.configuration_utils import WatermarkingConfig
    from genvc_amd.engine import WATERMARK_KWARGS, WatermarkSettings, watermark_settings
    assert WATERMARK_KWARGS == ("watermarking_config",)
    want = WatermarkSettings(0.25, 2.0, 15485863, "lefthash", 1)
    assert watermark_settings(dict(watermarking_config={}), V) == want
    assert watermark_settings(dict(watermarking_config=WatermarkingConfig()), V) == want
    assert watermark_settings(dict(watermarking_config=dict(bias=-1, hashing_key=7, seeding_scheme="selfhash", greenlist_ratio=0.5)), V) == \
        WatermarkSettings(0.5, -1.0, 7, "selfhash", 1)
    assert watermark_settings(dict(watermarking_config=dict(hashing_key=2 ** 63 - 1, bias=0)), V).hashing_key == 2 ** 63 - 1


@pytest.mark.parametrize("off", [{}, dict(watermarking_config=None)])
def test_off_spelling_passes_no_table(off):
    from genvc_amd.engine import GptEngine, watermark_settings
    assert watermark_settings(off, V) is None
    calls = []

    class Eng:
        def generate(self, *a, **k):
            calls.append("generate")

        def generate_wm(self, *a, **k):
            calls.append("generate_wm")
    GptEngine.generate_call(Eng(), torch.zeros(2, dtype=torch.int32), None, None, None, None, 0, 1, None, None, wm=None)
    assert calls == ["generate"]


BAD = [dict(greenlist_ratios=0.25), dict(seeding_scheme="righthash"), dict(greenlist_ratio=0.0), dict(greenlist_ratio=1.0),
       dict(greenlist_ratio=1.5), dict(greenlist_ratio=-0.1), dict(greenlist_ratio=float("nan")), dict(greenlist_ratio="0.25"),
       dict(greenlist_ratio=0.0005), dict(bias=float("inf")), dict(bias=float("nan")), dict(bias="2"), dict(hashing_key=1.5),
       dict(hashing_key=-1), dict(hashing_key=2 ** 63), dict(hashing_key="7"), dict(bias=True), dict(hashing_key=True),
       dict(greenlist_ratio=True), dict(context_width=True), dict(seeding_scheme=False), dict(context_width=1.0)]


@pytest.mark.parametrize("bad", BAD, ids=[f"{list(b)[0]}={list(b.values())[0]!r}" for b in BAD])
def test_argument_errors_are_value_errors(bad):
    from genvc_amd.engine import watermark_settings
    with pytest.raises(ValueError, match="watermarking_config"):
        watermark_settings(dict(watermarking_config=bad), V)
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="watermarking_config"):
        g.generate(cond, codes, top_k=15, watermarking_config=bad)
    with pytest.raises(ValueError, match="watermarking_config"):
        g.generate(cond, codes, do_sample=False, watermarking_config=bad)
    with pytest.raises(ValueError, match="watermarking_config"):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), top_k=15, watermarking_config=bad))


@pytest.mark.parametrize("bad", [True, False, 3, "lefthash", [("bias", 2.0)]])
def test_a_value_that_is_no_config_is_a_value_error(bad):
    from genvc_amd.engine import watermark_settings
    with pytest.raises(ValueError, match="watermarking_config"):
        watermark_settings(dict(watermarking_config=bad), V)


@pytest.mark.parametrize("scheme", ["lefthash", "selfhash"])
@pytest.mark.parametrize("width", [2, 0, 4])
def test_context_width_other_than_one_is_not_implemented_by_name(scheme, width):
    from genvc_amd.engine import watermark_settings
    with pytest.raises(NotImplementedError, match=f"context_width={width}"):
        watermark_settings(dict(watermarking_config=dict(seeding_scheme=scheme, context_width=width)), V)


def test_modes_refuse_by_name():
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    kw = dict(watermarking_config=dict(CFG))
    named = re.escape("watermarking_config with ")
    with pytest.raises(NotImplementedError, match=named + re.escape("beam search (num_beams=4)")):
        g.generate(cond, codes, num_beams=4, do_sample=False, **kw)
    with pytest.raises(NotImplementedError, match=named + "beam groups"):
        g.generate(cond, codes, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, do_sample=False, **kw)
    with pytest.raises(NotImplementedError, match=named + re.escape("contrastive search (penalty_alpha=0.6)")):
        g.generate(cond, codes, do_sample=False, top_k=4, penalty_alpha=0.6, **kw)
    for extra in (dict(do_sample=False), dict(speculative_sampling=True, top_k=15)):
        with pytest.raises(NotImplementedError, match=named + re.escape("assisted decoding (assistant_model)")):
            g.generate(cond, codes, assistant_model=cpu_gpt(), **kw, **extra)
        with pytest.raises(NotImplementedError, match=named + re.escape("prompt-lookup decoding (prompt_lookup_num_tokens)")):
            g.generate(cond, codes, prompt_lookup_num_tokens=4, **kw, **extra)
    with pytest.raises(NotImplementedError, match=named + "ras_window=4"):
        g.generate(cond, codes, top_k=15, ras_window=4, **kw)
    with pytest.raises(NotImplementedError, match=named + "ras_window=4"):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), top_k=15, ras_window=4, **kw))
    self_kw = dict(watermarking_config=dict(CFG, seeding_scheme="selfhash"))
    with pytest.raises(NotImplementedError, match="selfhash.*do_sample=False"):
        g.generate(cond, codes, do_sample=False, **self_kw)
    with pytest.raises(NotImplementedError, match="selfhash.*typical_p=0.9"):
        g.generate(cond, codes, top_k=15, typical_p=0.9, **self_kw)
    # the joint paths serve the mark on sampled rows; greedy rows raise by name (greedy search with the mark is GPT.generate's)
    for extra in (dict(top_k=1), dict(do_sample=False)):
        with pytest.raises(NotImplementedError, match=named + "greedy rows.*" + re.escape("the grouped path (generate_groups)")):
            g.generate_groups([(cond, codes)], **kw, **extra)
        with pytest.raises(NotImplementedError, match=named + "greedy rows.*" + re.escape("the rolling path (generate_rolling)")):
            g.generate_rolling([(cond, codes)], **kw, **extra)
        with pytest.raises(NotImplementedError, match=named + "greedy rows"):
            g.generate_groups([(cond, codes)], group_kwargs=[kw], **extra)
    with pytest.raises(NotImplementedError, match=named + "ras_window=4"):
        g.generate_groups([(cond, codes)], top_k=15, group_kwargs=[dict(kw, ras_window=4)])
    with pytest.raises(ValueError, match=re.escape("job_kwargs[0]: watermarking_config")):
        g.generate_rolling([(cond, codes)], top_k=15, job_kwargs=[dict(watermarking_config=dict(bias=float("nan")))])
    for call in (lambda: g.generate_groups([(cond, codes)], top_k=15, **kw), lambda: g.generate_rolling([(cond, codes)], top_k=15, **kw),
                 lambda: g.generate_groups([(cond, codes)], top_k=15, group_kwargs=[kw])):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):          # served: the call ends at the engine check
            call()


def test_per_item_dicts_carry_the_mark_with_the_sets():
    from genvc_amd import _lib
    from genvc_amd.engine import WarperSets, WatermarkSettings, check_proc_kwargs, logits_sets
    from genvc_amd.layers.gpt import _per_item_procs
    from genvc_amd.streaming import StreamSessions
    check_proc_kwargs(dict(watermarking_config=dict(CFG), min_p=0.1, presence_penalty=0.5), "row 0")
    with pytest.raises(ValueError, match="'watermarking_configs' is not a processor kwarg"):
        check_proc_kwargs(dict(watermarking_configs=dict(CFG)), "row 0")

    class Eng:          # an engine stand-in: one table address per key
        def __init__(self):
            self.asked, self.released = [], []

        def watermark_entry(self, s, hold=True):
            self.asked.append(s)
            return _lib.LogitsWatermark(4096 * (1 + s.hashing_key), s.bias, 0, 33, 0), s.hashing_key

        def watermark_release(self, key):
            self.released.append(key)
    eng = Eng()
    a, b = dict(CFG, hashing_key=1), dict(CFG, hashing_key=2)
    kws = [dict(watermarking_config=a), None, dict(watermarking_config=b, min_new_tokens=3), dict(watermarking_config=a),
           dict(typical_p=0.5), dict(watermarking_config=None), dict(watermarking_config=dict(a, bias=1.0))]
    ws = logits_sets(kws, 40, V, engine=eng)
    assert isinstance(ws, WarperSets) and ws.wm is not None and ws.pen is None
    assert list(ws.set_of_row) == [0, -1, 1, 0, 2, -1, 3] and ws.n_sets == 4 and ws.wm.n == 4
    assert [(m.table, m.bias) for m in ws.wm.wm] == [(8192, 2.0), (12288, 2.0), (None, 0.0), (8192, 1.0)]          # (a null table: off)
    assert [s.hashing_key for s in eng.asked] == [1, 2, 1]
    ws.wm.release()
    assert sorted(eng.released) == [1, 1, 2]
    assert logits_sets([dict(typical_p=0.5), None], 40, V).wm is None
    with pytest.raises(ValueError, match="needs the engine"):
        logits_sets([dict(watermarking_config=a)], 40, V)
    with pytest.raises(ValueError, match=r"row 1: watermarking_config"):
        logits_sets([None, dict(watermarking_config=dict(greenlist_ratio=2))], 40, V, engine=eng)
    merged = _per_item_procs(dict(watermarking_config=a), [None, dict(watermarking_config=None), dict(watermarking_config=b)], 3,
                             "job_kwargs", V)
    assert merged[0]["watermarking_config"] == a and merged[1]["watermarking_config"] is None and merged[2]["watermarking_config"] == b
    assert WatermarkSettings(0.25, 2.0, 1, "lefthash", 1) == eng.asked[0]
    sess = type("S", (), {"m": type("M", (), {"gpt": type("G", (), {"num_audio_tokens": V})()})()})()
    assert StreamSessions._procs(sess, dict(watermarking_config=a), {}, "open") == dict(watermarking_config=a)
    with pytest.raises(ValueError, match=r"open: watermarking_config"):
        StreamSessions._procs(sess, dict(watermarking_config=dict(hashing_key=-1)), {}, "open")


def test_sampling_with_top_k_1_points_to_greedy_search():
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="do_sample=False"):
        g.generate(cond, codes, top_k=1, watermarking_config=dict(CFG))
    with pytest.raises(ValueError, match="do_sample=False"):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), top_k=1, watermarking_config=dict(CFG)))


def test_served_calls_reach_the_engine_check():
    """greedy search with lefthash, sampling with either scheme, guidance and num_return_sequences are served, as is None: the call
    ends where every call on a GPT without an engine ends"""
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    for kw in (dict(watermarking_config=dict(CFG), do_sample=False), dict(watermarking_config=dict(CFG), top_k=15),
               dict(watermarking_config=dict(CFG, seeding_scheme="selfhash"), top_k=0, top_p=0.9), dict(watermarking_config=None),
               dict(watermarking_config=dict(CFG), guidance_scale=1.5, negative_cond_latents=cond),
               dict(watermarking_config=dict(CFG), num_return_sequences=2), dict(watermarking_config=dict(CFG), presence_penalty=0.5)):
        with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
            g.generate(cond, codes, **kw)


def test_engine_refuses_a_table_that_does_not_fit_its_sets():
    from genvc_amd import _lib
    from genvc_amd.engine import GptEngine, WarperSets, WatermarkTable
    m = (_lib.LogitsWatermark(0, 2.0, 0, 33, 0), None)
    with pytest.raises(ValueError, match="2 watermark entries for 1 sets"):
        GptEngine._wm_args(None, WatermarkTable([m, m]), None)
    assert len(GptEngine._wm_args(None, WatermarkTable([m]), WarperSets([None], [None], [0, 0]))) == 1


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------
def _run(script, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *flags], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)


def test_infer_flags():
    r = _run("infer.py", "--device", "cpu", "--help")
    assert r.returncode == 0 and all(f in r.stdout for f in ("--watermark_key", "--watermark_bias", "--watermark_ratio", "--watermark_scheme"))
    # good values pass the checks, with and without --streaming: the run ends at a later check of another flag
    for flags in (("--watermark_key", "7"), ("--watermark_key", "7", "--watermark_bias", "1.5", "--watermark_ratio", "0.5", "--streaming"),
                  ("--watermark_key", "7", "--watermark_scheme", "selfhash"), ("--watermark_key", "7", "--top_k", "1", "--greedy")):
        r = _run("infer.py", "--device", "cpu", *flags, "--min_p", "2")
        assert r.returncode != 0 and "bad processor flag: min_p" in r.stderr, r.stderr[-400:]
    for flags, msg in ((("--watermark_key", "-1"), "--watermark_key must be in [0, 2**63)"),
                       (("--watermark_key", "1.5"), "invalid int value"),
                       (("--watermark_key", "7", "--watermark_ratio", "1.0"), "--watermark_ratio must be in (0, 1)"),
                       (("--watermark_key", "7", "--watermark_ratio", "nan"), "--watermark_ratio must be in (0, 1)"),
                       (("--watermark_key", "7", "--watermark_bias", "inf"), "--watermark_bias must be finite"),
                       (("--watermark_key", "7", "--watermark_scheme", "righthash"), "invalid choice"),
                       (("--watermark_key", "7", "--top_k", "1"), "pass --greedy"),
                       (("--watermark_key", "7", "--num_beams", "4"), "does not combine with --num_beams"),
                       (("--watermark_key", "7", "--ras_window", "4"), "does not combine")):
        r = _run("infer.py", "--device", "cpu", *flags)
        assert r.returncode != 0 and msg in r.stderr, (flags, r.stderr[-400:])


def test_detect_script_flags():
    r = _run("scripts/detect_watermark.py", "--help")
    assert r.returncode == 0 and all(f in r.stdout for f in ("--tokens", "--watermark_key", "--watermark_ratio", "--watermark_scheme",
                                                             "--ignore_repeated_ngrams"))
    r = _run("scripts/detect_watermark.py", "--tokens", "nothing.npz", "--watermark_key", "7", "--watermark_ratio", "2")
    assert r.returncode != 0 and "greenlist_ratio" in r.stderr


# ---- 7. the C ABI -------------------------------------------------------------------------------------------------------------------
def test_struct_and_symbols():
    from genvc_amd import _lib
    assert C.sizeof(_lib.LogitsWatermark) == 24
    assert [(f, t) for f, t in _lib.LogitsWatermark._fields_] == [("table", C.c_void_p), ("bias", C.c_float), ("scheme", C.c_int32),
                                                                  ("words", C.c_int32), ("reserved", C.c_int32)]
    header = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    assert re.search(r"typedef struct gvc_logits_watermark \{\s*const uint32_t\* table;[^}]*float bias;[^}]*int32_t scheme;[^}]*"
                     r"int32_t words;[^}]*int32_t reserved;[^}]*\} gvc_logits_watermark;", header)
    assert (_lib.WM_LEFTHASH, _lib.WM_SELFHASH, _lib.WM_SELFHASH_TOP) == tuple(
        int(re.search(rf"#define {n}\s+(\d+)", header).group(1)) for n in ("GVC_WM_LEFTHASH", "GVC_WM_SELFHASH", "GVC_WM_SELFHASH_TOP"))
    src = open(os.path.join(ROOT, "genvc_amd", "csrc", "watermark.h")).read()
    assert int(re.search(r"kWmMaxScoreLen = (\d+)", src).group(1)) == _lib.WM_MAX_SCORE_LEN
    declared = set(re.findall(r"\b(gvc_[a-z0-9_]+)\s*\(", header))
    with open(_lib.LIB_PATH, "rb") as f:          # the built library: its dynamic string table names what it exports
        built = f.read()
    for s in SYMBOLS:
        assert s in declared, s
        assert s in _lib._SIGNATURES, s
        assert s in _lib.exported_symbols(), s
        assert s.encode() + b"\0" in built, f"{s} is not in {_lib.LIB_PATH}"
