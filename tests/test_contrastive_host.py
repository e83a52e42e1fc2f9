"""CPU: the contrastive-search restatement (tests/cs_oracle.py) against tests/golden/contrastive_search.npz (the loop driven on the
reference's own forward, scripts/make_contrastive_golden.py), the kwargs dispatch and validation of GPT.generate, and the new C ABI
symbols."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cs_oracle as CO                        # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "contrastive_search.npz")
SYMBOLS = ("gvc_gpt_prefill_hidden", "gvc_gpt_contrastive_generate", "gvc_gpt_contrastive_generate_proc", "gvc_gpt_warmup_contrastive")
TAGS = ["a", "b", "c", "d", "e"]


def case(gold, tag):
    """(weights, dims, cond, codes, K, rep, max_new, kw) of a fixture case"""
    margs = gcfg.DEFAULT_MODEL_ARGS if int(gold[f"{tag}_full"]) else gcfg.TINY_MODEL_ARGS
    dims = gcfg.gpt_dims(margs)
    w = synth.make_weights(int(gold[f"{tag}_seed"]), synth.gpt_weight_spec(dims))
    if float(gold[f"{tag}_stop_bias"]) != 0.0:
        w["mel_head.bias"][1025] = float(gold[f"{tag}_stop_bias"])
    B, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (B, Tc), 256)
    kw = {}
    if int(gold[f"{tag}_ngram"]):
        kw["no_repeat_ngram_size"] = int(gold[f"{tag}_ngram"])
    if int(gold[f"{tag}_min_new"]):
        kw["min_new_tokens"] = int(gold[f"{tag}_min_new"])
    return margs, w, dims, cond, codes, int(gold[f"{tag}_K"]), float(gold[f"{tag}_rep"]), int(gold[f"{tag}_max_new"]), kw


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_fixture(tag):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    gold = dict(np.load(GOLD))
    _, w, dims, cond, codes, K, rep, max_new, kw = case(gold, tag)
    for i in range(int(gold[f"{tag}_n"])):
        a = float(gold[f"{tag}_{i}_alpha"])
        r = CO.search(w, dims, cond, codes, K, a, rep, max_new, kw)
        assert np.array_equal(r["ids"], gold[f"{tag}_{i}_ids"])
        # the margin screens hold, stored and recomputed
        assert r["prob_gap"] >= 1e-3 and float(gold[f"{tag}_{i}_prob_gap"]) >= 1e-3
        assert r["score_gap"] >= 1e-4 and float(gold[f"{tag}_{i}_score_gap"]) >= 1e-4
        # ablation: the ranking changes the tokens (alpha = 0 is greedy decoding)
        assert r["off_top1"]
        greedy = CO.search(w, dims, cond, codes, K, 0.0, rep, max_new, kw)["ids"]
        assert greedy.shape != r["ids"].shape or not np.array_equal(greedy, r["ids"])
        # every processor kwarg the case sets changes its ids on its own (a device that dropped one could not reproduce the case)
        for key in kw:
            ids = CO.search(w, dims, cond, codes, K, a, rep, max_new, {k: v for k, v in kw.items() if k != key})["ids"]
            assert ids.shape != r["ids"].shape or not np.array_equal(ids, r["ids"]), key


def test_fixture_cases_cover_the_issue():
    gold = dict(np.load(GOLD))
    Ks = {t: int(gold[f"{t}_K"]) for t in TAGS}
    Bs = {t: int(gold[f"{t}_B"]) for t in TAGS}
    assert (Bs["a"], Ks["a"]) == (1, 2) and (Bs["b"], Ks["b"]) == (1, 4) and (Bs["c"], Ks["c"]) == (3, 2)
    rows = gold["c_0_ids"]
    stops = {int((r == 1025).argmax()) if (r == 1025).any() else -1 for r in rows}
    assert len(stops) >= 2                                       # ragged EOS
    assert int(gold["d_ngram"]) > 0 and int(gold["d_min_new"]) > 0 and float(gold["d_rep"]) == 1.0
    assert int(gold["e_full"]) == 1 and Ks["e"] == 4 and float(gold["e_rep"]) == 10.0
    assert int(gold["e_Tc"]) + 32 + 3 == 48                      # a 48-row prompt
    assert sorted(float(gold[f"e_{i}_alpha"]) for i in range(int(gold["e_n"]))) == [0.3, 0.6]


def test_contrastive_kwargs_dispatch():
    from genvc_amd.layers.gpt import _contrastive_kwargs
    assert _contrastive_kwargs(dict(do_sample=False, top_k=4, penalty_alpha=0.6)) == (4, 0.6, 1.0)
    assert _contrastive_kwargs(dict(do_sample=False, top_k=4, penalty_alpha=0.6, repetition_penalty=10.0))[2] == 10.0
    # 4.33's test: top_k > 1, do_sample False, penalty_alpha > 0; top_k absent = GenerationConfig's 50 (beyond the device's 16)
    assert _contrastive_kwargs(dict(do_sample=True, top_k=4, penalty_alpha=0.6)) is None
    assert _contrastive_kwargs(dict(top_k=4, penalty_alpha=0.6)) is None          # (this build's generate samples by default)
    assert _contrastive_kwargs(dict(do_sample=False, top_k=1, penalty_alpha=0.6)) is None
    assert _contrastive_kwargs(dict(do_sample=False, top_k=4, penalty_alpha=0.0)) is None
    assert _contrastive_kwargs(dict(do_sample=False, top_k=4)) is None
    assert _contrastive_kwargs(dict(do_sample=False, top_k=None, penalty_alpha=0.6)) is None     # 4.33: an explicit None fails the test
    with pytest.raises(NotImplementedError, match="16"):
        _contrastive_kwargs(dict(do_sample=False, penalty_alpha=0.6))
    with pytest.raises(NotImplementedError, match="16"):
        _contrastive_kwargs(dict(do_sample=False, top_k=17, penalty_alpha=0.6))
    assert _contrastive_kwargs(dict(do_sample=False, top_k=16, penalty_alpha=0.6, num_beams=4))[0] == 16   # before num_beams
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite"):
            _contrastive_kwargs(dict(do_sample=False, top_k=4, penalty_alpha=bad))
    with pytest.raises(ValueError, match="num_return_sequences"):
        _contrastive_kwargs(dict(do_sample=False, top_k=4, penalty_alpha=0.6, num_return_sequences=2))
    with pytest.raises(ValueError, match=r"init_gpt_for_inference\(max_slots"):
        _contrastive_kwargs(dict(do_sample=False, top_k=4, penalty_alpha=0.6), B=3, max_slots=8)
    assert _contrastive_kwargs(dict(do_sample=False, top_k=4, penalty_alpha=0.6), B=2, max_slots=8)[0] == 4


def test_refused_paths_name_themselves():
    """the one-row-per-stream entry points refuse the contrastive kwargs before they touch the device, naming themselves -- also with
    top_k absent (GenerationConfig's 50, which GPT.generate would refuse for K > 16 instead) and with a K the device would take"""
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"])
    cond, codes = torch.zeros(1, 32, a["gpt_n_model_channels"]), torch.zeros(1, 5, dtype=torch.long)
    for kw in (dict(do_sample=False, top_k=4, penalty_alpha=0.6), dict(do_sample=False, penalty_alpha=0.6)):
        with pytest.raises(NotImplementedError, match=re.escape("streaming (get_generator)")):
            next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))
        with pytest.raises(NotImplementedError, match=re.escape("grouped (generate_groups)")):
            g.generate_groups([(cond, codes)], **kw)
        with pytest.raises(NotImplementedError, match=re.escape("rolling (generate_rolling)")):
            g.generate_rolling([(cond, codes)], **kw)
    # sampling with penalty_alpha is not refused: it reaches the engine check (no engine on this CPU-only module)
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
        g.generate_groups([(cond, codes)], do_sample=True, top_k=4, penalty_alpha=0.6)


def test_new_symbols_declared_and_exported():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    assert "gvc_contrastive_state" in hdr
    if os.path.exists(_lib.LIB_PATH):
        import subprocess
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s
