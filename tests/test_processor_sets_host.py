"""CPU: per-row logits processor sets (include/genvc_hip.h: gvc_sample_proc_sets / gvc_gpt_generate_proc_sets) -- the host packing
(engine.logits_processor_sets), the validation of group_kwargs / job_kwargs / generate_kwargs, the exported symbols, and
tests/proc_oracle.py applied row by row through the packed index against the per-set results."""
import os
import subprocess
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import proc_oracle as PO                      # noqa: E402
from genvc_amd import _lib                    # noqa: E402
from genvc_amd.engine import PROC_KWARGS, logits_processor_sets, logits_processors   # noqa: E402

EOS, V = 1025, 1026


def test_identical_dicts_share_a_set_and_none_rows_map_to_minus_one():
    a = dict(no_repeat_ngram_size=2, suppress_tokens=[5, 3])
    b = dict(min_new_tokens=4)
    ps = logits_processor_sets([a, None, dict(a), b, {}, dict(suppress_tokens=(3, 5), no_repeat_ngram_size=2), None, b], 40, V)
    assert ps.n_sets == 2 and len(ps) == 8
    assert list(ps.set_of_row) == [0, -1, 0, 1, -1, 0, -1, 1]
    assert ps.sets[0].no_repeat_ngram_size == 2 and ps.sets[0].n_suppress == 2 and ps.sets[0].prompt_len == 40
    assert ps.sets[1].min_new_tokens == 4
    # every row without a processor, or with every processor at its default: no sets at all
    assert logits_processor_sets([None, {}, dict(min_new_tokens=0, suppress_tokens=None)], 40, V) is None


def test_rows_with_different_prompts_get_sets_of_their_own():
    k = dict(min_new_tokens=3)
    ps = logits_processor_sets([k, k, k, None], [40, 52, 40, 7], V)
    assert ps.n_sets == 2 and list(ps.set_of_row) == [0, 1, 0, -1]
    assert (ps.sets[0].prompt_len, ps.sets[1].prompt_len) == (40, 52)


def test_index_range_and_set_count_are_checked():
    with pytest.raises(ValueError, match="1..64"):
        logits_processor_sets([None] * 65, 4, V)
    with pytest.raises(ValueError, match="1..64"):
        logits_processor_sets([], 4, V)
    with pytest.raises(ValueError, match="prompt lengths"):
        logits_processor_sets([None, None], [3, 4, 5], V)
    ps = logits_processor_sets([dict(suppress_tokens=[i]) for i in range(64)], 9, V)
    assert ps.n_sets == 64 and list(ps.set_of_row) == list(range(64))
    assert all(-1 <= k < ps.n_sets for k in ps.set_of_row)


@pytest.mark.parametrize("bad,match", [
    (dict(no_repeat_ngram_size=9), "no_repeat_ngram_size"),
    (dict(min_new_tokens=-1), "min_new_tokens"),
    (dict(suppress_tokens=[V]), "suppress_tokens"),
    (dict(exponential_decay_length_penalty=(1, 0.0)), "exponential_decay_length_penalty"),
    (dict(min_p=1.5), "min_p"),
    (dict(top_k=15), "'top_k' is not a processor kwarg"),
])
def test_malformed_row_names_the_row(bad, match):
    with pytest.raises(ValueError, match=match) as e:
        logits_processor_sets([None, dict(min_new_tokens=2), bad], 10, V)
    assert str(e.value).startswith("row 2:")


def _tiny_gpt():
    from genvc_amd import config as gcfg
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    return GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
               max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
               max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
               start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
               num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
               stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])


def test_group_and_job_kwargs_accept_processor_kwargs_only():
    """checked before any device work: an unknown key, a wrong count or a malformed setting raises ValueError naming the item"""
    g = _tiny_gpt()
    groups = [(None, torch.zeros(1, 4)), (None, torch.zeros(2, 4))]
    with pytest.raises(ValueError, match=r"group_kwargs\[1\]: 'temperature'"):
        g.generate_groups(groups, group_kwargs=[None, dict(temperature=0.5)], top_k=1)
    with pytest.raises(ValueError, match=r"group_kwargs\[0\]: no_repeat_ngram_size"):
        g.generate_groups(groups, group_kwargs=[dict(no_repeat_ngram_size=20), None], top_k=1)
    with pytest.raises(ValueError, match="2 items"):
        g.generate_groups(groups, group_kwargs=[None], top_k=1)
    with pytest.raises(ValueError, match=r"job_kwargs\[0\]: 'seed'"):
        g.generate_rolling(groups, job_kwargs=[dict(seed=3), None], top_k=1)
    with pytest.raises(ValueError, match=r"job_kwargs\[1\]: suppress_tokens"):
        g.generate_rolling(groups, job_kwargs=[None, dict(suppress_tokens=[-2])], top_k=1)
    with pytest.raises(NotImplementedError):           # beams keep raising as before
        g.generate_groups(groups, group_kwargs=[None, None], num_beams=2)


def test_session_generate_kwargs_accept_processor_kwargs_only():
    from genvc_amd.streaming import StreamSessions
    ss = StreamSessions.__new__(StreamSessions)
    ss.m = types.SimpleNamespace(gpt=types.SimpleNamespace(num_audio_tokens=V))
    base = ss._procs(dict(no_repeat_ngram_size=2), {}, "StreamSessions(generate_kwargs=...)")
    assert base == dict(no_repeat_ngram_size=2)
    assert ss._procs(dict(min_new_tokens=4, no_repeat_ngram_size=None), base, "open") == dict(no_repeat_ngram_size=2, min_new_tokens=4)
    assert ss._procs(None, {}, "open") is None
    with pytest.raises(ValueError, match="open: 'top_k' is not a processor kwarg"):
        ss._procs(dict(top_k=1), base, "open")
    with pytest.raises(ValueError, match="open: min_p"):
        ss._procs(dict(min_p=2.0), base, "open")


def test_new_symbols_are_exported():
    assert {"gvc_sample_proc_sets", "gvc_gpt_generate_proc_sets"} <= set(_lib.exported_symbols())
    assert os.path.exists(_lib.LIB_PATH), "build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    have = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"gvc_sample_proc_sets", "gvc_gpt_generate_proc_sets"} <= have


def _unpack(pr):
    """a packed gvc_logits_processors -> the processor kwargs it restates (for proc_oracle.process)"""
    def toks(words):
        return [i for i in range(V) if (words[i >> 5] >> (i & 31)) & 1]
    kw = {}
    if pr.no_repeat_ngram_size:
        kw["no_repeat_ngram_size"] = pr.no_repeat_ngram_size
    if pr.min_length:
        kw["min_length"] = pr.min_length
    if pr.min_new_tokens:
        kw["min_new_tokens"] = pr.min_new_tokens
    if pr.decay_factor > 0:
        kw["exponential_decay_length_penalty"] = (pr.decay_start, float(pr.decay_factor))
    if pr.n_suppress:
        kw["suppress_tokens"] = toks(pr.suppress)
    if pr.n_begin_suppress:
        kw["begin_suppress_tokens"] = toks(pr.begin_suppress)
    return kw


def test_oracle_row_by_row_through_the_index_equals_the_per_set_results():
    """a mixed batch: every row processed with the set its index names (unpacked from the packed struct) equals the rows of that set
    in a run of the set over the whole batch, and a -1 row is untouched"""
    gen = torch.Generator().manual_seed(11)
    B, plen = 12, 20
    kws = [dict(no_repeat_ngram_size=2), dict(min_new_tokens=6, suppress_tokens=[7, 9]), None,
           dict(begin_suppress_tokens=[4], exponential_decay_length_penalty=(1, 1.25)), dict(min_length=plen + 3, suppress_tokens=[2])]
    row_kw = [kws[b % 5] for b in range(B)]
    ps = logits_processor_sets(row_kw, plen, V, sampling=False)
    assert ps.n_sets == 4
    scores = torch.randn(B, V, generator=gen) * 3
    rows = []
    for b in range(B):
        L = plen + (b % 4)                           # lengths plen .. plen + 3: begin_suppress, min_length and the decay all act
        row = torch.randint(0, 12, (L,), generator=gen).tolist()
        rows.append(row)
    mixed = torch.stack([scores[b] if ps.set_of_row[b] < 0 else
                         PO.process(scores[b], rows[b], plen, _unpack(ps.sets[ps.set_of_row[b]]), EOS) for b in range(B)])
    for k in range(ps.n_sets):
        whole = torch.stack([PO.process(scores[b], rows[b], plen, _unpack(ps.sets[k]), EOS) for b in range(B)])
        mine = [b for b in range(B) if ps.set_of_row[b] == k]
        assert mine and torch.equal(mixed[mine], whole[mine]), k
        # the set is the one its rows asked for
        assert all(torch.equal(whole[b], PO.process(scores[b], rows[b], plen, row_kw[b], EOS)) for b in mine), k
    none = [b for b in range(B) if ps.set_of_row[b] == -1]
    assert none and torch.equal(mixed[none], scores[none])
    assert set(PO.KEYS) == set(PROC_KWARGS)
    assert logits_processors(kws[0], plen, V) is not None
