"""Deferred decode of a call's last token (csrc/gpt.hip: the generation loop of one stream on the one-launch step runs
[decode the pending token, sample] and leaves the last sampled token pending for the slot).  Every case compares a deferring context
with one created under GVC_DEFER_DECODE=0 (the eager order [sample, decode]) on the same weights.  The comparisons are bit-exact: both
orders run the same kernels on the same inputs, only the call in which a decode runs differs."""
import pytest
import torch

from genvc_amd import config as gcfg
from genvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
GREEDY = dict(gcfg.DEFAULT_SAMPLING, top_k=1)
TOPK50 = dict(gcfg.DEFAULT_SAMPLING, top_k=50)
WIDE2 = dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2)          # d = 1024, H = 4, L = 2: the width the one-launch step serves
N_MAX = 64


@pytest.fixture
def pair(monkeypatch):
    """(dims, deferring engine, eager engine) on the same weights; the switch is read when a context is created"""
    from genvc_amd.engine import GptEngine
    torch.cuda.empty_cache()
    dims = gcfg.gpt_dims(WIDE2)
    w = synth.make_weights(3, synth.gpt_weight_spec(dims), device=DEV)
    monkeypatch.delenv("GVC_DEFER_DECODE", raising=False)
    d = GptEngine(dims, max_slots=4, max_rows=2048)
    d.bind(w)
    monkeypatch.setenv("GVC_DEFER_DECODE", "0")
    e = GptEngine(dims, max_slots=4, max_rows=2048)
    e.bind(w)
    monkeypatch.delenv("GVC_DEFER_DECODE")
    yield dims, d, e
    d.close()
    e.close()
    torch.cuda.empty_cache()


class Run:
    """one stream of one engine: its prompt, its slot and the buffers of the reference loop"""

    def __init__(self, eng, dims, slot=0, seed_in=300, sampling=GREEDY, seed=0, proc_kw=None):
        from genvc_amd.engine import logits_processors, sample_params
        self.eng, self.dims = eng, dims
        cond = synth.uniform(seed_in, "cond_latents", (1, 32, dims["d_model"]), 1.0)
        codes = synth.integers(seed_in, "content_codes", (1, 13), 256)
        self.prefix = eng.prefix_embeddings(cond.to(DEV), codes.to(DEV).int())
        self.P = self.prefix.shape[1]
        self.slots = torch.tensor([slot], device=DEV, dtype=torch.int32)
        self.sp = sample_params(sampling, dims["num_audio_tokens"], dims["stop_audio_token"], seed)
        self.proc = None
        if proc_kw:
            self.proc = logits_processors(proc_kw, self.P + 1, dims["num_audio_tokens"], sampling=sampling["top_k"] != 1)
        self.start()

    def start(self, n_cached=0):
        P, d = self.P, self.dims["d_model"]
        self.ids = torch.ones(1, P + 1 + N_MAX + 8, device=DEV, dtype=torch.int32)
        self.ids[:, P] = self.dims["start_audio_token"]
        self.ids_len = torch.full((1,), P + 1, device=DEV, dtype=torch.int32)
        self.fin = torch.zeros(1, device=DEV, dtype=torch.int32)
        self.toks = torch.full((1, N_MAX), -1, device=DEV, dtype=torch.int32)
        self.lats = torch.zeros(1, N_MAX, d, device=DEV)
        self.done = 0
        self.eng.prefill(self.slots, self.prefix, want_outputs=False, n_cached=n_cached)

    def clone_to(self, slot):
        """the same stream continued in another slot (after a kv_fanout): copies of the loop's buffers"""
        import copy
        r = copy.copy(self)
        r.slots = torch.tensor([slot], device=DEV, dtype=torch.int32)
        for k in ("ids", "ids_len", "fin", "toks", "lats"):
            setattr(r, k, getattr(self, k).clone())
        return r

    def gen(self, n):
        self.eng.generate(self.slots, self.ids, self.ids_len, self.fin, self.sp, self.done, n, self.toks, self.lats,
                          max_keys=self.P + 1 + N_MAX, proc=self.proc)
        self.done += n

    def state(self):
        torch.cuda.synchronize()
        self.eng.health()
        return dict(tokens_out=self.toks.cpu(), latents_out=self.lats.cpu(), ids=self.ids.cpu(), ids_len=self.ids_len.cpu(),
                    finished=self.fin.cpu())


def assert_same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs between the deferring and the eager order"


CALLS = {
    "3x8": (8, 8, 8),
    "1_3_8_24": (1, 3, 8, 24),
    "24_8_3_1": (24, 8, 3, 1),
    "zeros_between": (3, 0, 8, 0, 0, 1, 24, 0),
    "zero_first": (0, 1, 0, 3, 8),
}
SAMPLERS = {
    "greedy": dict(sampling=GREEDY),
    "top_k50": dict(sampling=TOPK50, seed=7),
    "greedy_proc": dict(sampling=GREEDY, proc_kw=dict(no_repeat_ngram_size=2, min_new_tokens=6)),
}


@pytest.mark.parametrize("sampler", list(SAMPLERS))
@pytest.mark.parametrize("calls", list(CALLS))
def test_calls_of_any_length_give_the_eager_outputs(pair, calls, sampler):
    """1. one stream generated in calls of 1, 3, 8 and 24 steps, 0-step calls in between: tokens_out, latents_out, ids, ids_len and
    finished are those of the eager order"""
    dims, d, e = pair
    got, want = Run(d, dims, **SAMPLERS[sampler]), Run(e, dims, **SAMPLERS[sampler])
    for n in CALLS[calls]:
        got.gen(n)
        want.gen(n)
        assert_same(got.state(), want.state(), f"after a call of {n} steps ({got.done} so far)")
    assert d.decode_variant() == 3 and e.decode_variant() == 3, "not on the one-launch step: nothing was deferred"


def test_decode_step_after_a_deferring_generate(pair):
    """2. an explicit decode step settles the pending token first: same logits and latent for a chosen token"""
    dims, d, e = pair
    got, want = Run(d, dims), Run(e, dims)
    tok = torch.tensor([5], device=DEV, dtype=torch.int32)
    out = []
    for r in (got, want):
        r.gen(8)
        r.gen(3)
        out.append(r.eng.decode_step(r.slots, tok))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    # ... and a second one (nothing pending any more)
    out = [r.eng.decode_step(r.slots, tok) for r in (got, want)]
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("sampler", ["greedy", "top_k50"])
def test_kv_fanout_carries_the_pending_token(pair, sampler):
    """3. a fan-out after a deferring generate copies the pending token: source and destination continue alike, and as the eager order"""
    dims, d, e = pair
    res = []
    for eng in (d, e):
        src = Run(eng, dims, **SAMPLERS[sampler])
        src.gen(8)
        src.gen(1)
        eng.kv_fanout(src.slots, torch.tensor([2], device=DEV, dtype=torch.int32))
        dst = src.clone_to(2)
        for n in (8, 3):
            src.gen(n)
            dst.gen(n)
        res.append((src.state(), dst.state()))
    assert_same(res[0][0], res[0][1], "source vs destination (deferring)")
    assert_same(res[0][0], res[1][0], "source")
    assert_same(res[0][1], res[1][1], "destination")


def test_batched_call_over_a_pending_and_a_fresh_slot(pair):
    """4. B = 2 over a slot with a pending token and a freshly prefilled one: the batched call settles the first before it starts"""
    dims, d, e = pair
    res = []
    for eng in (d, e):
        a = Run(eng, dims, slot=0)
        a.gen(8)
        b = Run(eng, dims, slot=1, seed_in=301)
        slots = torch.cat([a.slots, b.slots])
        ids = torch.cat([a.ids, b.ids])
        ids_len = torch.cat([a.ids_len, b.ids_len])
        fin = torch.cat([a.fin, b.fin])
        toks = torch.cat([a.toks, b.toks])
        lats = torch.cat([a.lats, b.lats])
        for i0, n in ((8, 8), (16, 5)):
            eng.generate(slots, ids, ids_len, fin, a.sp, i0, n, toks, lats, max_keys=a.P + 1 + N_MAX)
        # ... and back to one stream, which defers again
        eng.generate(slots[:1], ids[:1], ids_len[:1], fin[:1], a.sp, 21, 8, toks[:1], lats[:1], max_keys=a.P + 1 + N_MAX)
        torch.cuda.synchronize()
        eng.health()
        res.append(dict(tokens_out=toks.cpu(), latents_out=lats.cpu(), ids=ids.cpu(), ids_len=ids_len.cpu(), finished=fin.cpu()))
    assert_same(res[0], res[1], "B = 2 after a deferring call")


def test_cached_prefill_drops_the_pending_token(pair):
    """5. prefill_cached(n_cached = 32) right after a deferring generate, then a full chunk"""
    dims, d, e = pair
    got, want = Run(d, dims), Run(e, dims)
    for r in (got, want):
        for _ in range(3):
            r.gen(8)
    assert_same(got.state(), want.state(), "first chunk")
    for r in (got, want):
        r.start(n_cached=32)
        for _ in range(3):
            r.gen(8)
    assert_same(got.state(), want.state(), "chunk after the cached prefill")


def test_executed_step_counter(pair):
    """6. a prefill followed by 3 x 8 steps executes 23 one-stream steps, a following cached-prefill chunk 23 more; 24 and 24 with the
    switch off"""
    dims, d, e = pair
    for eng, per_chunk in ((d, 23), (e, 24)):
        base = eng.one_stream_steps()
        assert base >= 0
        r = Run(eng, dims)
        for _ in range(3):
            r.gen(8)
        assert eng.one_stream_steps() - base == per_chunk
        r.start(n_cached=32)
        for _ in range(3):
            r.gen(8)
        assert eng.one_stream_steps() - base == 2 * per_chunk
        assert eng.decode_variant() == 3


def test_warmup_covers_the_deferring_graphs(pair):
    """7. after warmup(), a prefill followed by 3 x 8 steps does no lazy initialisation"""
    dims, d, _ = pair
    r = Run(d, dims)
    d.warmup(1, r.P + 1 + N_MAX, 1)
    before = d.lazy_inits()
    r.start()
    for _ in range(3):
        r.gen(8)
    r.state()
    assert d.decode_variant() == 3
    assert d.lazy_inits() == before
