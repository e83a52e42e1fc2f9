"""GPU: the sampler and generation entry-point families are wrappers over one internal path (csrc/sampler.hip: sample_once,
csrc/gpt.hip: generate_impl, engine.py: _sample / _generate / generate_call).  An entry called with its extra options null must give
exactly the narrower entry's result, an option passed through a wider entry exactly what the narrower entry gives for it, and
generate_call with an entry's options exactly that entry's result -- tokens and latents, torch.equal.  Row counts 1 (one stream),
2 and 5 (the rows step); 11 steps per call: one unrolled graph of eight steps plus three single ones."""
import pytest
import torch

from genvc_amd import config as gcfg
from genvc_amd import synth
from genvc_amd.engine import GptEngine, ProcessorSets, WarperSets, logits_bias, logits_processors, sample_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS, V = 1025, 1026
N = 11
SEED = 5
MODES = dict(greedy=dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=1),
             sampling=dict(repetition_penalty=1.0, temperature=0.8, top_p=1.0, top_k=50))
PROC = dict(min_new_tokens=4, no_repeat_ngram_size=2)


@pytest.fixture(scope="module")
def eng():
    dims = gcfg.gpt_dims(gcfg.TINY_MODEL_ARGS)
    e = GptEngine(dims, max_slots=10)
    e.bind(synth.make_weights(3, synth.gpt_weight_spec(dims), device=DEV))
    yield e
    e.close()
    torch.cuda.empty_cache()


def _keys(samp, B):
    """every row carrying the call's settings and the key the plain call gives it: (seed, row, 0)"""
    return [dict(samp, seed=SEED, rng_row=r, rng_step0=0) for r in range(B)]


class _Loop:
    """one prefix over B rows; run(fn) prefills the same slots again (the unconditional ones too) and hands fn fresh loop buffers"""

    def __init__(self, eng, B):
        d = eng.dims["d_model"]
        cond = synth.uniform(300 + B, "cond_latents", (B, 32, d), 1.0).to(DEV)
        codes = synth.integers(300 + B, "content_codes", (B, 13), 256).to(DEV).int()
        self.eng, self.B = eng, B
        self.prefix = eng.prefix_embeddings(cond, codes)
        self.P = int(self.prefix.shape[1])
        self.slots = torch.arange(B, device=DEV, dtype=torch.int32)
        self.uslots = torch.arange(B, 2 * B, device=DEV, dtype=torch.int32)
        self.mk = self.P + 1 + N

    def run(self, fn):
        eng, B, P = self.eng, self.B, self.P
        eng.prefill(self.slots, self.prefix, want_outputs=False)
        eng.prefill(self.uslots, self.prefix, want_outputs=False)
        ids = torch.ones(B, P + 1 + N + 8, device=DEV, dtype=torch.int32)
        ids[:, P] = eng.dims["start_audio_token"]
        ids_len = torch.full((B,), P + 1, device=DEV, dtype=torch.int32)
        fin = torch.zeros(B, device=DEV, dtype=torch.int32)
        toks = torch.full((B, N), EOS, device=DEV, dtype=torch.int32)
        lats = torch.zeros(B, N, eng.d, device=DEV)
        fn(self.slots, ids, ids_len, fin, toks, lats)
        torch.cuda.synchronize()
        eng.health()
        return toks.cpu(), lats.cpu()


def _same(got, want, what):
    assert torch.equal(got[0], want[0]), f"{what}: tokens differ"
    assert torch.equal(got[1], want[1]), f"{what}: latents differ"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [1, 2, 5])
def test_generate_entries_with_null_options_are_the_narrower_entry(eng, B, mode):
    samp = MODES[mode]
    L = _Loop(eng, B)
    mk = L.mk
    p = sample_params(samp, V, EOS, SEED)
    keys = _keys(samp, B)
    proc = logits_processors(PROC, L.P + 1, V, sampling=mode == "sampling")
    off = ProcessorSets([proc], [-1] * B)
    base = L.run(lambda s, i, n, f, t, l: eng.generate(s, i, n, f, p, 0, N, t, l, max_keys=mk))
    assert int((base[0] != EOS).sum()) > 0
    rungs = {
        "generate_scores(no uncond, no sets, no buffers)":
            lambda s, i, n, f, t, l: eng.generate_scores(s, None, 1.0, i, n, f, p, None, 0, N, t, l, max_keys=mk),
        "generate_bias(bias None)":
            lambda s, i, n, f, t, l: eng.generate_bias(s, None, 1.0, i, n, f, p, None, None, 0, N, t, l, max_keys=mk),
        "generate_call(no options)":
            lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, p, 0, N, t, l, max_keys=mk),
        "generate_rows(the call's settings and keys)":
            lambda s, i, n, f, t, l: eng.generate_rows(s, i, n, f, keys, 0, N, t, l, max_keys=mk),
        "generate_proc_sets(every index -1)":
            lambda s, i, n, f, t, l: eng.generate_proc_sets(s, i, n, f, p, off, 0, N, t, l, max_keys=mk),
        "generate_call(rows)":
            lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, None, 0, N, t, l, max_keys=mk, rows=keys),
        "generate_call(sets, every index -1)":
            lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, p, 0, N, t, l, max_keys=mk, sets=off),
    }
    for what, fn in rungs.items():
        _same(L.run(fn), base, f"B={B} {mode}: {what}")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [1, 2, 5])
def test_one_processor_set_through_every_entry(eng, B, mode):
    samp = MODES[mode]
    L = _Loop(eng, B)
    mk = L.mk
    p = sample_params(samp, V, EOS, SEED)
    keys = _keys(samp, B)
    proc = logits_processors(PROC, L.P + 1, V, sampling=mode == "sampling")
    one = ProcessorSets([proc], [0] * B)
    warp = WarperSets.one(proc, None, B)
    base = L.run(lambda s, i, n, f, t, l: eng.generate(s, i, n, f, p, 0, N, t, l, max_keys=mk, proc=proc))
    rungs = {
        "generate_proc_sets(one set for all rows)":
            lambda s, i, n, f, t, l: eng.generate_proc_sets(s, i, n, f, p, one, 0, N, t, l, max_keys=mk),
        "generate_warp(WarperSets.one(proc, None))":
            lambda s, i, n, f, t, l: eng.generate_warp(s, i, n, f, p, warp, 0, N, t, l, max_keys=mk),
        "generate_scores(the same sets)":
            lambda s, i, n, f, t, l: eng.generate_scores(s, None, 1.0, i, n, f, p, warp, 0, N, t, l, max_keys=mk),
        "generate_bias(the same sets, bias None)":
            lambda s, i, n, f, t, l: eng.generate_bias(s, None, 1.0, i, n, f, p, warp, None, 0, N, t, l, max_keys=mk),
        "generate_rows(proc)":
            lambda s, i, n, f, t, l: eng.generate_rows(s, i, n, f, keys, 0, N, t, l, max_keys=mk, proc=proc),
        "generate_call(proc)":
            lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, p, 0, N, t, l, max_keys=mk, proc=proc),
        "generate_call(rows, proc)":
            lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, None, 0, N, t, l, max_keys=mk, rows=keys, proc=proc),
        "generate_call(ProcessorSets)":
            lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, p, 0, N, t, l, max_keys=mk, sets=one),
        "generate_call(WarperSets)":
            lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, p, 0, N, t, l, max_keys=mk, sets=warp),
    }
    for what, fn in rungs.items():
        _same(L.run(fn), base, f"B={B} {mode}: {what}")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("B", [1, 2, 5])
def test_generate_call_reaches_the_wide_entries(eng, B, mode):
    """the rungs generate_call picks by a real option: score buffers, a sequence bias, guidance -- each against the entry called by name,
    with the call-wide processors handed over as `proc` on one side and as the entry's one-set WarperSets on the other"""
    samp = MODES[mode]
    L = _Loop(eng, B)
    mk = L.mk
    p = sample_params(samp, V, EOS, SEED)
    do_sample = mode == "sampling"
    proc = logits_processors(PROC, L.P + 1, V, sampling=do_sample)
    warp = WarperSets.one(proc, None, B)
    bias = logits_bias(dict(renormalize_logits=True, bad_words_ids=[[7, 9]]), L.P + 1, N, V, EOS)
    bufs = [torch.zeros(B, N, V, device=DEV) for _ in range(4)]
    base = L.run(lambda s, i, n, f, t, l: eng.generate(s, i, n, f, p, 0, N, t, l, max_keys=mk, proc=proc))
    want = L.run(lambda s, i, n, f, t, l: eng.generate_scores(s, None, 1.0, i, n, f, p, warp, 0, N, t, l, scores_out=bufs[0],
                                                               logits_out=bufs[1], do_sample=do_sample, max_keys=mk))
    got = L.run(lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, p, 0, N, t, l, max_keys=mk, proc=proc, scores_out=bufs[2],
                                                            logits_out=bufs[3], do_sample=do_sample))
    _same(want, base, f"B={B} {mode}: generate_scores with buffers")
    _same(got, base, f"B={B} {mode}: generate_call(scores_out, logits_out)")
    assert torch.equal(bufs[0], bufs[2]) and torch.equal(bufs[1], bufs[3]) and bool(bufs[1].abs().sum() > 0)
    want = L.run(lambda s, i, n, f, t, l: eng.generate_bias(s, None, 1.0, i, n, f, p, warp, bias, 0, N, t, l, max_keys=mk))
    got = L.run(lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, p, 0, N, t, l, max_keys=mk, proc=proc, bias=bias))
    _same(got, want, f"B={B} {mode}: generate_call(bias)")
    want = L.run(lambda s, i, n, f, t, l: eng.generate_cfg(s, L.uslots, 1.5, i, n, f, p, warp, 0, N, t, l, max_keys=mk))
    got = L.run(lambda s, i, n, f, t, l: eng.generate_call(s, i, n, f, p, 0, N, t, l, max_keys=mk, proc=proc, uncond_slots=L.uslots,
                                                            scale=1.5))
    _same(got, want, f"B={B} {mode}: generate_call(uncond_slots)")
    wide = L.run(lambda s, i, n, f, t, l: eng.generate_bias(s, L.uslots, 1.5, i, n, f, p, warp, None, 0, N, t, l, max_keys=mk))
    _same(wide, want, f"B={B} {mode}: generate_bias(uncond_slots, bias None) against generate_cfg")


@pytest.mark.parametrize("mode", list(MODES))
def test_sample_entries_ladder(eng, mode):
    samp = MODES[mode]
    gen = torch.Generator().manual_seed(11)
    B, n0 = 5, 9
    logits = (torch.randn(B, V, generator=gen) * 3).to(DEV).contiguous()
    ids0 = torch.randint(0, 1024, (B, n0 + 16), generator=gen).int()
    ids0[:, n0 - 2:n0] = ids0[:, 2:4]                   # the rows end with a pair they held before: the n-gram ban has a hit to make
    logits[torch.arange(B), ids0[:, 4].long().to(DEV)] = 40.0        # ... on the token every row would otherwise take
    p = sample_params(samp, V, EOS, SEED)
    keys = _keys(samp, B)
    proc = logits_processors(PROC, n0 - 2, V, sampling=mode == "sampling")
    off, one, warp = ProcessorSets([proc], [-1] * B), ProcessorSets([proc], [0] * B), WarperSets.one(proc, None, B)

    def call(fn, *a, **k):
        ids = ids0.clone().to(DEV)
        ids_len = torch.full((B,), n0, device=DEV, dtype=torch.int32)
        fin = torch.zeros(B, device=DEV, dtype=torch.int32)
        return fn(logits, ids, ids_len, fin, *a, **k).cpu()
    for step in (0, 3):
        base = call(eng.sample, p, step)
        rows = [dict(k, rng_step0=0) for k in keys]
        assert torch.equal(call(eng.sample_rows, rows, step), base), (step, "sample_rows")
        assert torch.equal(call(eng.sample_proc_sets, p, off, step), base), (step, "sample_proc_sets, every index -1")
        assert torch.equal(call(eng.sample_proc_sets, p, off, step, rows=rows), base), (step, "sample_proc_sets, rows, every index -1")
        assert torch.equal(call(eng.sample_bias, p, None, step), base), (step, "sample_bias(None), no sets")
        assert torch.equal(call(eng.sample_bias, p, None, step, rows=rows), base), (step, "sample_bias(None), rows")
        with_proc = call(eng.sample_proc, p, proc, step)
        assert not torch.equal(with_proc, base), "the processor set changes nothing: the ladder would compare plain calls"
        assert torch.equal(call(eng.sample_proc, p, proc, step, rows=rows), with_proc), (step, "sample_proc, rows")
        assert torch.equal(call(eng.sample_proc_sets, p, one, step), with_proc), (step, "sample_proc_sets, one set")
        assert torch.equal(call(eng.sample_warp, p, warp, step), with_proc), (step, "sample_warp")
        assert torch.equal(call(eng.sample_warp, p, warp, step, rows=rows), with_proc), (step, "sample_warp, rows")
        assert torch.equal(call(eng.sample_bias, p, None, step, sets=warp), with_proc), (step, "sample_bias(None), WarperSets")
        assert torch.equal(call(eng.sample_bias, p, None, step, sets=one), with_proc), (step, "sample_bias(None), ProcessorSets")
