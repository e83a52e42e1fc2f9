"""CPU: sequence_bias / bad_words_ids / forced_eos_token_id / forced_bos_token_id / renormalize_logits of GPT.generate
(include/genvc_hip.h: gvc_logits_bias).  tests/bias_oracle.py's per-row restatement against the installed transformers' own classes,
executed in _get_logits_processor's order; engine.logits_bias's packing and validation; the C ABI struct and symbols; the modes and
paths that refuse the kwargs by name."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bias_oracle as BI                      # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gvc_sample_bias", "gvc_gpt_generate_bias")
D = gcfg.TINY_MODEL_ARGS["gpt_n_model_channels"]
V, EOS = 1026, 1025
NINF = -float("inf")


# ---- 1. the restatement against the executed HF chain --------------------------------------------------------------------------------
def both(logits, row, plen, kw, rep=1.0, max_new=12):
    """(bias_oracle.process, the executed HF chain) on one row"""
    mine = BI.process(logits, row, plen, kw, EOS, rep=rep, max_new=max_new)
    hf = BI.run_chain(BI.hf_chain(kw, plen, EOS, rep, max_new), torch.tensor([row]), logits[None])[0]
    return mine, hf


def same(mine, hf, what):
    gi, hi = torch.isinf(mine) & (mine < 0), torch.isinf(hf) & (hf < 0)
    assert torch.equal(gi, hi), f"{what}: the -inf pattern differs"
    assert not bool(torch.isnan(hf).any()) and torch.equal(mine[~hi], hf[~hi]), f"{what}: {float((mine - hf)[~hi].abs().max()):.3e}"


def rows():
    gen = torch.Generator().manual_seed(31)
    return [torch.randn(V, generator=gen) * 3.0 for _ in range(4)]


def test_the_chain_is_built_in_the_documented_order():
    kw = dict(sequence_bias={(9,): -1.0}, bad_words_ids=[[6, EOS]], forced_eos_token_id=EOS, forced_bos_token_id=3, renormalize_logits=True,
              no_repeat_ngram_size=2, min_length=3, min_new_tokens=2, exponential_decay_length_penalty=(2, 1.1), suppress_tokens=[4],
              begin_suppress_tokens=[5])
    chain = BI.hf_chain(kw, 6, EOS, 2.0, 12, sampling=dict(temperature=0.8, top_k=8))
    assert [type(p).__name__ for p in chain] == BI.ORDER
    assert chain[7].max_length == 18 and chain[7].eos_token_id.tolist() == [EOS]


@pytest.mark.parametrize("rep", [1.0, 2.0])
def test_sequence_bias_rows(rep):
    plen = 4
    row = [1, 1, 1, 1024, 7]                                      # the prompt is (1, 1, 1, 1024): `1, 1024, 7` straddles its end
    cases = {
        "a prefix across the prompt boundary": {(1, 1024, 7, 9): 1.5},
        "the same prefix, one id off": {(1, 1023, 7, 9): 1.5},
        "two entries ending in one token": {(7, 9): 0.5, (1024, 7, 9): 0.25},
        "a length-1 and a longer entry on one token": {(7, 9): 0.5, (9,): -1.0},
        "a -inf bias": {(11,): NINF, (7, 12): NINF, (7, 9): 0.3},
        "an entry as long as the row, and one longer": {(1, 1, 1024, 7, 9): 2.0, (1, 1, 1, 1024, 7, 10): 2.0},
        "id 0 in the dict form": {(0,): -3.0, (7, 0): 1.0},
    }
    for what, sb in cases.items():
        for logits in rows():
            mine, hf = both(logits, row, plen, dict(sequence_bias=sb), rep)
            same(mine, hf, what)
    # ... and they do what their names say
    lg = rows()[0]
    hit = BI.process(lg, row, plen, dict(sequence_bias=cases["a prefix across the prompt boundary"]), EOS)
    miss = BI.process(lg, row, plen, dict(sequence_bias=cases["the same prefix, one id off"]), EOS)
    assert float(hit[9]) == float(lg[9] + 1.5) and torch.equal(miss, lg)
    long_ = BI.process(lg, row, plen, dict(sequence_bias=cases["an entry as long as the row, and one longer"]), EOS)
    assert float(long_[9]) == float(lg[9] + 2.0) and float(long_[10]) == float(lg[10])
    # both input forms give the same row
    as_list = [[[7, 9], 0.5], [[9], -1.0]]
    a, hf = both(lg, row, plen, dict(sequence_bias=as_list), rep)
    same(a, hf, "list form")
    assert torch.equal(a, BI.process(lg, row, plen, dict(sequence_bias={(7, 9): 0.5, (9,): -1.0}), EOS, rep=rep))


def test_the_bias_comes_before_the_penalty():
    """a seen token at +0.5 with bias -1.0 at penalty 2 scores (0.5 - 1.0) * 2 = -1.0; behind the penalty it would be 0.25 - 1.0"""
    lg = torch.full((V,), -5.0)
    lg[7] = 0.5
    mine, hf = both(lg, [1, 1024, 7], 2, dict(sequence_bias={(7,): -1.0}), rep=2.0)
    same(mine, hf, "order")
    assert float(hf[7]) == -1.0


def test_bad_words_rows():
    kw = dict(bad_words_ids=[[EOS], [6, EOS], [1024, 5, 8], [13]])
    for tail, banned in (([1024, 6], True), ([1024, 5], False)):
        for logits in rows():
            mine, hf = both(logits, [1, 1] + tail, 3, kw, rep=2.0)
            same(mine, hf, f"tail {tail}")
            # [6, 1025] bans the stop token behind a 6; the bare [1025] is dropped, so nothing else ever bans it
            assert bool(torch.isinf(hf[EOS])) == banned and bool(torch.isinf(hf[13])) and bool(torch.isinf(hf[8])) == (tail[-1] == 5)
    # with the n-gram ban and the other processors around it
    more = dict(kw, no_repeat_ngram_size=2, min_new_tokens=1, suppress_tokens=[40], sequence_bias={(6, 41): 0.7})
    mine, hf = both(rows()[1], [1, 1024, 6, 9, 6], 2, more, rep=2.0)
    same(mine, hf, "with n-gram, min_new_tokens, suppress and a bias")
    assert bool(torch.isinf(hf[9])) and bool(torch.isinf(hf[EOS])) and bool(torch.isinf(hf[40]))


@pytest.mark.parametrize("extra", [{}, dict(min_new_tokens=12, no_repeat_ngram_size=1, bad_words_ids=[[EOS, EOS], [7, EOS]],
                                            sequence_bias={(EOS,): -4.0}),
                                   dict(exponential_decay_length_penalty=(2, 1.2), sequence_bias={(EOS,): -4.0}, suppress_tokens=[3])])
def test_forced_eos_rows(extra):
    """alone; with every ban of the stop token ahead of it in the list (min_new_tokens, the n-gram ban, a bad word: the forced EOS
    overrides them); and with the decay and suppress_tokens behind it (the decay of a forced 0.0 is 0.0)"""
    plen, max_new = 3, 6
    kw = dict(forced_eos_token_id=EOS, **extra)
    for n_new in (max_new - 2, max_new - 1, max_new):              # one step either side of len == max_length - 1
        row = [1, 1, 1024] + [7] * n_new
        for logits in rows()[:2]:
            mine, hf = both(logits, row, plen, kw, rep=2.0, max_new=max_new)
            same(mine, hf, f"{n_new} new tokens")
            fired = int(torch.isfinite(hf).sum()) == 1 and float(hf[EOS]) == 0.0
            assert fired == (n_new == max_new - 1)


def test_forced_bos_leaves_rows_alone():
    lg = rows()[2]
    for row in ([1, 1024], [1, 1, 1024, 5]):
        mine, hf = both(lg, row, 2, dict(forced_bos_token_id=3))
        same(mine, hf, "forced BOS")
        assert torch.equal(hf, lg)


def test_renormalized_rows():
    lg = rows()[3]
    kw = dict(renormalize_logits=True, suppress_tokens=[3, 4], sequence_bias={(9,): NINF})
    mine, hf = both(lg, [1, 1024, 7], 2, kw, rep=2.0)
    gi = torch.isinf(hf)
    assert torch.equal(gi, torch.isinf(mine)) and int(gi.sum()) == 3
    assert float((mine - hf)[~gi].abs().max()) <= 1e-6 and abs(float(torch.logsumexp(hf, -1))) <= 1e-5


# ---- 2. packing ---------------------------------------------------------------------------------------------------------------------
def pack(kw, plen=40, max_new=12):
    from genvc_amd.engine import logits_bias
    return logits_bias(kw, plen, max_new, V, EOS)


def unpack(z):
    n = z.n_bias + z.n_ban
    return [(tuple(z.ids[e][:z.len[e]]), z.bias[e]) for e in range(n)]


def test_packing():
    from genvc_amd import _lib
    sb = {(3, 4, 5): 1.5, (EOS,): -2.0, (8, 9): 0.25, (7,): NINF}
    z = pack(dict(sequence_bias=sb, bad_words_ids=[[EOS], [6, EOS], [13]], forced_eos_token_id=EOS, renormalize_logits=True))
    assert isinstance(z, _lib.LogitsBias)
    assert (z.n_bias, z.n_ban, z.force_eos_at, z.renormalize, z.prompt_len, list(z.reserved)) == (4, 2, 12, 1, 40, [0, 0, 0])
    # length-1 entries first, dict order otherwise; then the bad words without the bare [eos]
    assert unpack(z) == [((EOS,), -2.0), ((7,), NINF), ((3, 4, 5), 1.5), ((8, 9), 0.25), ((6, EOS), NINF), ((13,), NINF)]
    assert all(x == 0 for e in range(6, 32) for x in z.ids[e]) and list(z.len[6:]) == [0] * 26
    as_list = pack(dict(sequence_bias=[[list(k), v] for k, v in sb.items()], bad_words_ids=[[6, EOS], [13]], forced_eos_token_id=EOS,
                        renormalize_logits=True))
    assert ctypes.string_at(ctypes.addressof(z), ctypes.sizeof(z)) == ctypes.string_at(ctypes.addressof(as_list), ctypes.sizeof(z))
    # id 0 goes in both forms (HF's list form refuses it: the one deviation)
    assert unpack(pack(dict(sequence_bias=[[[0], 1.0]]))) == unpack(pack(dict(sequence_bias={(0,): 1.0}))) == [((0,), 1.0)]
    # each kwarg alone
    assert pack(dict(forced_eos_token_id=EOS), max_new=7).force_eos_at == 7 and pack(dict(forced_eos_token_id=[EOS])).force_eos_at == 12
    assert pack(dict(renormalize_logits=True)).renormalize == 1 and pack(dict(bad_words_ids=[[5, 6]])).n_ban == 1


@pytest.mark.parametrize("kw", [{}, dict(sequence_bias=None, bad_words_ids=None, forced_eos_token_id=None, renormalize_logits=None),
                                dict(sequence_bias={}), dict(sequence_bias=[]), dict(bad_words_ids=[]), dict(renormalize_logits=False),
                                dict(bad_words_ids=[[EOS]]), dict(forced_bos_token_id=3),
                                dict(sequence_bias={}, bad_words_ids=[[EOS]], renormalize_logits=False, forced_bos_token_id=1024)])
def test_off_spellings_pack_to_none(kw):
    assert pack(kw) is None


def test_malformed_settings_raise():
    many = {(i, i + 1): 0.5 for i in range(20)}
    with pytest.raises(ValueError, match="33 entries.*32"):
        pack(dict(sequence_bias=many, bad_words_ids=[[i] for i in range(100, 113)]))
    assert pack(dict(sequence_bias=many, bad_words_ids=[[i] for i in range(100, 112)])).n_ban == 12           # 32 fit
    with pytest.raises(ValueError, match="sequence_bias.*9 ids.*8"):
        pack(dict(sequence_bias={tuple(range(9)): 1.0}))
    with pytest.raises(ValueError, match="bad_words_ids.*9 ids.*8"):
        pack(dict(bad_words_ids=[list(range(9))]))
    with pytest.raises(ValueError, match=r"sequence_bias: token 1026 outside \[0, 1026\)"):
        pack(dict(sequence_bias={(3, 1026): 1.0}))
    with pytest.raises(ValueError, match=r"bad_words_ids: token -1 outside"):
        pack(dict(bad_words_ids=[[-1]]))
    with pytest.raises(ValueError, match="sequence_bias.*finite or -inf"):
        pack(dict(sequence_bias={(3,): float("nan")}))
    with pytest.raises(ValueError, match="sequence_bias.*finite or -inf"):
        pack(dict(sequence_bias={(3,): float("inf")}))
    with pytest.raises(ValueError, match="sequence_bias.*empty|sequence_bias.*0 ids"):
        pack(dict(sequence_bias={(): 1.0}))
    with pytest.raises(ValueError, match=r"forced_eos_token_id=5 must be the model's stop token 1025"):
        pack(dict(forced_eos_token_id=5))
    with pytest.raises(ValueError, match="forced_eos_token_id=1025 with the stop token suppressed"):
        pack(dict(forced_eos_token_id=EOS, suppress_tokens=[3, EOS]))
    with pytest.raises(ValueError, match="renormalize_logits must be a bool"):
        pack(dict(renormalize_logits=1))


def test_struct_layout_and_symbols():
    from genvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genvc_hip.h")).read()
    body = re.search(r"typedef struct gvc_logits_bias \{(.*?)\} gvc_logits_bias;", hdr, re.S).group(1)
    caps = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (GVC_BIAS_MAX_\w+) (\d+)", hdr)}
    assert caps == dict(GVC_BIAS_MAX_SEQS=32, GVC_BIAS_MAX_LEN=8) == dict(GVC_BIAS_MAX_SEQS=_lib.BIAS_MAX_SEQS, GVC_BIAS_MAX_LEN=_lib.BIAS_MAX_LEN)
    # every member is 4 bytes wide: the size is 4 x the number of elements the header declares
    words, names = 0, []
    for typ, name, dims in re.findall(r"^\s*(int32_t|float)\s+(\w+)((?:\[\w+\])*);", body, re.M):
        n = 1
        for d in re.findall(r"\[(\w+)\]", dims):
            n *= caps[d] if d in caps else int(d)
        words += n
        names.append(name)
    assert names == [f[0] for f in _lib.LogitsBias._fields_]
    assert ctypes.sizeof(_lib.LogitsBias) == 4 * words == 1312
    assert _lib.LogitsBias.ids.offset == 32 + 4 * 32 * 2 and _lib.LogitsBias.len.offset == 32
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\(", hdr), s
        assert s in _lib.exported_symbols()
    if os.path.exists(_lib.LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        have = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for s in SYMBOLS:
            assert s in have, s
    # gvc_sample_warp + bias, gvc_gpt_generate_scores + bias; the entry points that were there keep their signatures
    sig = _lib._SIGNATURES
    assert len(sig["gvc_sample_bias"][1]) == len(sig["gvc_sample_warp"][1]) + 1 == 16
    assert len(sig["gvc_gpt_generate_bias"][1]) == len(sig["gvc_gpt_generate_scores"][1]) + 1 == 28
    assert ctypes.sizeof(_lib.LogitsProcessors) == 312 and ctypes.sizeof(_lib.LogitsWarpers) == 16 and ctypes.sizeof(_lib.SampleParams) == 32


def test_engine_names():
    from genvc_amd import engine as E
    assert E.BIAS_KWARGS == ("sequence_bias", "bad_words_ids", "forced_eos_token_id", "forced_bos_token_id", "renormalize_logits")
    assert not set(E.BIAS_KWARGS) & (set(E.PROC_KWARGS) | set(E.WARP_KWARGS))
    assert callable(E.GptEngine.sample_bias) and callable(E.GptEngine.generate_bias)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def cpu_gpt(max_slots=16):
    from genvc_amd.layers.gpt import GPT
    a = gcfg.TINY_MODEL_ARGS
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"])
    g.max_slots = max_slots
    return g


ON = [("sequence_bias", {(EOS,): -2.0}), ("bad_words_ids", [[5, 6]]), ("forced_eos_token_id", EOS), ("renormalize_logits", True)]


@pytest.mark.parametrize("key,value", ON, ids=[k for k, _ in ON])
def test_modes_and_paths_refuse_by_name(key, value):
    from genvc_amd.inference import inference_utils as IU
    from genvc_amd.streaming import StreamSessions
    g = cpu_gpt()
    cond, codes = torch.zeros(1, 32, D), torch.zeros(1, 5, dtype=torch.long)
    kw = {key: value}
    named = re.escape(f"{key}={value!r} is not served with ")
    with pytest.raises(NotImplementedError, match=named + re.escape("beam search (num_beams=4)")):
        g.generate(cond, codes, num_beams=4, do_sample=False, **kw)
    with pytest.raises(NotImplementedError, match=named + "beam groups"):
        g.generate(cond, codes, num_beams=4, num_beam_groups=2, diversity_penalty=0.5, do_sample=False, **kw)
    with pytest.raises(NotImplementedError, match=named + re.escape("contrastive search (penalty_alpha=0.6)")):
        g.generate(cond, codes, do_sample=False, top_k=4, penalty_alpha=0.6, **kw)
    with pytest.raises(NotImplementedError, match=named + re.escape("the streaming (get_generator) path")):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **kw))
    with pytest.raises(NotImplementedError, match=named + re.escape("the grouped (generate_groups) path")):
        g.generate_groups([(cond, codes)], **kw)
    with pytest.raises(NotImplementedError, match=named + re.escape("the rolling (generate_rolling) path")):
        g.generate_rolling([(cond, codes)], top_k=1, **kw)
    with pytest.raises(NotImplementedError, match=named + re.escape("the session (StreamSessions, open) path")):
        StreamSessions._procs(object(), dict(kw), {}, "open")
    with pytest.raises(NotImplementedError, match=named + ".*" + re.escape("infer.py --streaming")):
        IU.synthesize_utt_streaming(object(), torch.zeros(1, 16000), torch.zeros(1, 24000), generate_kwargs=dict(kw))
    # an off spelling reaches the engine check as ever
    off = {key: {} if key == "sequence_bias" else [] if key == "bad_words_ids" else None if key == "forced_eos_token_id" else False}
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
        g.generate_groups([(cond, codes)], **off)
    with pytest.raises(RuntimeError, match="init_gpt_for_inference"):
        next(g.get_generator(torch.ones(1, 40, dtype=torch.long), **off))


def test_per_row_dicts_keep_their_value_error():
    from genvc_amd.engine import check_proc_kwargs, logits_sets
    from genvc_amd.layers.gpt import _per_item_procs
    for key, value in ON:
        with pytest.raises(ValueError, match=f"row 1: '{key}' is not a processor kwarg"):
            logits_sets([None, {key: value}], 40, V)
        with pytest.raises(ValueError, match=re.escape(f"group_kwargs[0]: '{key}' is not a processor kwarg")):
            _per_item_procs({}, [{key: value}], 1, "group_kwargs", V)
        with pytest.raises(ValueError, match="is not a processor kwarg"):
            check_proc_kwargs({key: value}, "job_kwargs[2]")


def _infer(*flags):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--device", "cpu", *flags], capture_output=True, text=True,
                          env=env, cwd=ROOT)


def test_infer_flags():
    r = _infer("--streaming", "--sequence_bias", "1025=-2.0")
    assert r.returncode != 0 and "--forced_eos are not on the streaming path (--streaming)" in r.stderr
    r = _infer("--bad_words_ids", "5,6", "--num_beams", "4")
    assert r.returncode != 0 and "do not combine with --num_beams" in r.stderr
    r = _infer("--sequence_bias", "5,x=1")
    assert r.returncode != 0 and "--sequence_bias takes IDS=VALUE" in r.stderr
    r = _infer("--sequence_bias", "5,2000=1.0")
    assert r.returncode != 0 and "bad processor flag: sequence_bias: token 2000 outside" in r.stderr
