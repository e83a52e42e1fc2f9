"""GPU: per-row sampling keys and settings (include/genvc_hip.h gvc_row_sampling, gvc_sample_rows, gvc_gpt_generate_rows) and the
paths built on them: sampled joint decodes (GPT.generate_groups), sampled rolling decodes (GPT.generate_rolling, convert_offline
rolling=True) and per-session sampling in StreamSessions."""
import numpy as np
import pytest
import torch

from genvc_amd import config as gcfg
from genvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
SAMP = dict(repetition_penalty=2.0, temperature=0.85, top_p=0.85)      # the reference's defaults (configs/genVC_train_configs.py)
_cache = {}


def wide_engine():
    """GenVC's width (d_model 1024, 4 heads of 256) with two layers and 16 KV slots: one stream decodes on the one-launch step, 2..16
    on the one-launch rows step"""
    from genvc_amd.engine import GptEngine
    if "wide" not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        dims = gcfg.gpt_dims(dict(gcfg.DEFAULT_MODEL_ARGS, gpt_layers=2))
        w = synth.make_weights(3, synth.gpt_weight_spec(dims), device=DEV)
        eng = GptEngine(dims, max_slots=16, max_rows=1024)
        eng.bind(w)
        _cache["wide"] = (dims, w, eng)
    return _cache["wide"]


def tiny_model(max_slots=16):
    from genvc_amd.inference.model_init import model_init_synthetic
    key = ("tiny", max_slots)
    if key not in _cache:
        _cache.clear()
        torch.cuda.empty_cache()
        _cache[key] = model_init_synthetic(gcfg.default_config(tiny=True), seed=5, device=DEV, max_slots=max_slots)[0]
    return _cache[key]


def _draw(scores, u):
    """oracle.sample_from_scores for one row with the uniform u, and the draw's relative distance to the nearest CDF boundary"""
    kept = torch.isfinite(scores)
    e = torch.where(kept, torch.exp(scores - scores[kept].max()), torch.zeros_like(scores))
    cdf = torch.cumsum(e.double(), 0)
    total = float(cdf[-1])
    target = float(np.float32(u)) * total
    hit = torch.nonzero((cdf >= target) & kept)
    tok = int(hit[0]) if len(hit) else int(torch.nonzero(kept)[-1])
    margin = float((cdf[kept] - target).abs().min()) / total
    return tok, margin


def _row(top_k, top_p=0.85, temperature=0.85, repetition_penalty=2.0, seed=0, rng_row=0, rng_step0=0):
    return dict(top_k=top_k, top_p=top_p, temperature=temperature, repetition_penalty=repetition_penalty, seed=seed, rng_row=rng_row,
                rng_step0=rng_step0)


def test_sample_rows_mixed_settings_match_oracle():
    """gvc_sample_rows: every row its own processors and key; each equals oracle.process_logits + rng_uniform(seed, rng_step0 + step,
    rng_row) on draws screened away from CDF boundaries; greedy rows equal k_sample_greedy's token"""
    from genvc_amd.engine import sample_params
    from oracle import genvc_oracle as O
    dims, _, eng = wide_engine()
    V, B, step, S = 1026, 16, 3, 96
    logits = synth.uniform(41, "logits", (B, V), 2.0)
    hist = synth.integers(42, "ids", (B, S), V).long()
    lens = [20 + 5 * b for b in range(B)]
    ks, ps, ts, rps = (1, 15, 50, 0), (0.85, 1.0), (0.85, 1.0, 0.7), (2.0, 1.0, 1.5)
    rows = [_row(ks[b % 4], ps[b % 2], ts[b % 3], rps[b % 3], seed=1000 + 17 * b, rng_row=(b * 5) % 7, rng_step0=11 * b) for b in range(B)]
    expect, screened = [], 0
    for b, r in enumerate(rows):
        sc = O.process_logits(logits[b:b + 1], hist[b:b + 1, :lens[b]], r["repetition_penalty"], r["temperature"], r["top_k"], r["top_p"])[0]
        if r["top_k"] == 1:
            expect.append(int(torch.argmax(sc)))
            continue
        for _ in range(50):               # CPU screen: a key whose draw lies clear of every CDF boundary (no GPU run is repeated)
            tok, margin = _draw(sc, O.rng_uniform(r["seed"], r["rng_step0"] + step, r["rng_row"]))
            if margin > 1e-4:
                break
            r["seed"] += 1
        assert margin > 1e-4, (b, margin)
        screened += 1
        expect.append(tok)
    assert screened == 12

    def run(rs, n=B):
        ids = torch.zeros(n, 128, dtype=torch.int32, device=DEV)
        ids[:, :S] = hist[:n].to(DEV).int()
        ids_len = torch.tensor(lens[:n], dtype=torch.int32, device=DEV)
        fin = torch.zeros(n, dtype=torch.int32, device=DEV)
        tok = eng.sample_rows(logits[:n].to(DEV), ids, ids_len, fin, rs, step)
        assert ids_len.cpu().tolist() == [x + 1 for x in lens[:n]]
        return tok.cpu().tolist(), ids
    got, ids = run(rows)
    assert got == expect
    assert [int(ids[b, lens[b]]) for b in range(B)] == expect
    # greedy rows: the token k_sample_greedy gives them (all-greedy keyed call, and gvc_sample at top_k = 1 row by row)
    greedy = [dict(r, top_k=1) for r in rows]
    g_all, _ = run(greedy)
    for b in range(B):
        ids = torch.zeros(1, 128, dtype=torch.int32, device=DEV)
        ids[:, :S] = hist[b:b + 1].to(DEV).int()
        p = sample_params(dict(rows[b], top_k=1), V, 1025, seed=0)
        t = eng.sample(logits[b:b + 1].to(DEV), ids, torch.tensor([lens[b]], dtype=torch.int32, device=DEV),
                       torch.zeros(1, dtype=torch.int32, device=DEV), p, step)
        assert int(t) == g_all[b], b
        if rows[b]["top_k"] == 1:
            assert got[b] == g_all[b], b
    # a finished row emits the pad token whatever its key
    ids = torch.zeros(2, 128, dtype=torch.int32, device=DEV)
    fin = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    t = eng.sample_rows(logits[:2].to(DEV), ids, torch.full((2,), 4, dtype=torch.int32, device=DEV), fin, rows[:2], step)
    assert int(t[0]) == 1025


def _prefill_all(eng, dims, B, n_codes=13):
    cond = synth.uniform(300, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(301, "content_codes", (B, n_codes), 256).to(DEV).int()
    prefix = eng.prefix_embeddings(cond, codes)
    slots = torch.arange(B, device=DEV, dtype=torch.int32)
    eng.reset(slots)
    eng.prefill(slots, prefix, want_outputs=False)
    return prefix, slots


def test_rows_step_logits_do_not_depend_on_the_number_of_rows():
    """the gate of the joint sampled decode: on the rows step a slot's logits are bit-identical whether gvc_gpt_decode_step runs it among
    5, 8 or 16 rows?  Where it holds, generate_groups may decode sampled classes jointly by default; where it does not, the joint sampled
    decode stays opt-in (joint_sampling=True).  The default in layers/gpt.py records the outcome and this test pins it to the measurement"""
    from genvc_amd.layers.gpt import JOINT_SAMPLING_DEFAULT
    dims, _, eng = wide_engine()
    tok = synth.integers(302, "tok", (16,), 1024).to(DEV).int()
    outs = {}
    for B in (5, 8, 16):
        _, slots = _prefill_all(eng, dims, 16)
        n0 = eng.rows_step_launches()
        lg, lat = eng.decode_step(slots[:B].contiguous(), tok[:B].contiguous())
        torch.cuda.synchronize()
        assert eng.rows_step_launches() > n0                     # the one-launch rows step served it
        outs[B] = (lg[:5].cpu(), lat[:5].cpu())
    diffs = {B: (float((outs[B][0] - outs[5][0]).abs().max()), float((outs[B][1] - outs[5][1]).abs().max())) for B in (8, 16)}
    print(f"rows step, rows 0..4 among 5 rows vs 8 / 16 rows: max |d logits|, max |d latent| = {diffs}")
    same = all(torch.equal(outs[B][0], outs[5][0]) and torch.equal(outs[B][1], outs[5][1]) for B in (8, 16))
    assert same == JOINT_SAMPLING_DEFAULT


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("top_k", [1, 15])
def test_generate_rows_with_identity_keys_equals_generate(B, top_k):
    """rows[b] = {p's settings, p.seed, b, i0}: gvc_gpt_generate_rows is gvc_gpt_generate bit for bit (tokens and latents), on the same
    decode step (B = 1: the one-launch step at d = 1024; B = 8: the rows step)"""
    from genvc_amd.engine import sample_params
    dims, _, eng = wide_engine()
    d, n, seed = dims["d_model"], 20, 77
    res = []
    for keyed in (False, True):
        prefix, slots = _prefill_all(eng, dims, B)
        P = prefix.shape[1]
        ids = torch.ones(B, P + 1 + n + 8, device=DEV, dtype=torch.int32)
        ids[:, P] = dims["start_audio_token"]
        ids_len = torch.full((B,), P + 1, device=DEV, dtype=torch.int32)
        fin = torch.zeros(B, device=DEV, dtype=torch.int32)
        toks = torch.zeros(B, n, device=DEV, dtype=torch.int32)
        lats = torch.zeros(B, n, d, device=DEV)
        samp = dict(SAMP, top_k=top_k)
        done = 0
        for step_n in (3, 9, 8):           # three calls: i0 = 0, 3, 12 (graphs of eight steps and single steps)
            if keyed:
                eng.generate_rows(slots, ids, ids_len, fin, [_row(top_k, seed=seed, rng_row=b, rng_step0=done, **SAMP) for b in range(B)],
                                  done, step_n, toks, lats, max_keys=P + 1 + done + step_n)
            else:
                eng.generate(slots, ids, ids_len, fin, sample_params(samp, 1026, 1025, seed), done, step_n, toks, lats,
                             max_keys=P + 1 + done + step_n)
            done += step_n
        torch.cuda.synchronize()
        eng.health()
        res.append((toks.cpu(), lats.cpu(), eng.decode_variant()))
    assert res[0][2] == res[1][2] == (3 if B == 1 else 5)
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_generate_rows_jobs_with_own_seeds_equal_their_solo_runs_and_the_oracle():
    """two jobs (5 and 6 rows) with their own seeds in ONE generate_rows call: each equals that job decoded alone and
    oracle.generate(..., seed=s) for it (seeds screened on the CPU so that no draw lies within 1e-4 of a CDF boundary)"""
    from oracle import genvc_oracle as O
    dims, w, eng = wide_engine()
    wc = {k: v.cpu() for k, v in w.items()}
    d, n = dims["d_model"], 10
    samp = dict(SAMP, top_k=15)
    jobs = []
    for j, (b, tc, seed0) in enumerate(((5, 13, 11), (6, 9, 500))):
        cond = synth.uniform(310 + j, "cond_latents", (b, 32, d), 1.0)
        codes = synth.integers(320 + j, "content_codes", (b, tc), 256)
        _, ids0 = O.compute_embeddings(wc, dims, cond, codes)
        for seed in range(seed0, seed0 + 8):        # CPU screen of the job's key
            toks, _, lg = O.generate(wc, dims, cond, codes, samp, max_new=n, seed=seed, stop_on_eos=False)
            margin = 1.0
            for i in range(toks.shape[1]):
                ids = torch.cat([ids0, toks[:, :i]], 1)
                sc = O.process_logits(lg[i], ids, samp["repetition_penalty"], samp["temperature"], samp["top_k"], samp["top_p"])
                for r in range(b):
                    margin = min(margin, _draw(sc[r], O.rng_uniform(seed, i, r))[1])
            if margin > 1e-4:
                break
        assert margin > 1e-4, (j, margin)
        jobs.append(dict(cond=cond.to(DEV), codes=codes.to(DEV).int(), seed=seed, expect=toks))

    def run(sel):
        prefixes = [eng.prefix_embeddings(jobs[j]["cond"], jobs[j]["codes"]) for j in sel]
        B = sum(p.shape[0] for p in prefixes)
        W = max(p.shape[1] for p in prefixes) + 1 + n + 8
        slots = torch.arange(B, device=DEV, dtype=torch.int32)
        eng.reset(slots)
        ids = torch.ones(B, W, device=DEV, dtype=torch.int32)
        ids_len = torch.empty(B, device=DEV, dtype=torch.int32)
        rows, r0 = [], 0
        for j, p in zip(sel, prefixes):
            b, P = p.shape[0], p.shape[1]
            eng.prefill(slots[r0:r0 + b].contiguous(), p, want_outputs=False)
            ids[r0:r0 + b, P] = dims["start_audio_token"]
            ids_len[r0:r0 + b] = P + 1
            rows += [_row(15, seed=jobs[j]["seed"], rng_row=r, rng_step0=0, **SAMP) for r in range(b)]
            r0 += b
        fin = torch.zeros(B, device=DEV, dtype=torch.int32)
        toks = torch.zeros(B, n, device=DEV, dtype=torch.int32)
        eng.generate_rows(slots, ids, ids_len, fin, rows, 0, n, toks, None, max_keys=W - 8)
        torch.cuda.synchronize()
        eng.health()
        return toks.cpu().long()
    both = run([0, 1])
    alone = [run([0]), run([1])]
    assert torch.equal(both[:5], alone[0]) and torch.equal(both[5:], alone[1])
    assert torch.equal(both[:5], jobs[0]["expect"]) and torch.equal(both[5:], jobs[1]["expect"])


KW = dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0, do_sample=True, num_beams=1)


def _groups(m, layout):
    d = m.gpt.model_dim
    cond = synth.uniform(71, "cond", (1, 32, d), 1.0).to(DEV)
    return [(cond.expand(B, -1, -1).contiguous(), synth.integers(90 + i, "codes", (B, Tc), 256).to(DEV)) for i, (B, Tc) in enumerate(layout)]


def test_generate_groups_samples_jointly_and_equals_generate_per_class():
    """top_k 15, joint_sampling=True: the classes decode in ONE joint decode (groups_stats) and each class equals generate(seed=its class
    seed); several class layouts, ragged budgets, explicit class_seeds; the default runs them one after another with the same tokens"""
    m = tiny_model()
    g = m.gpt
    for layout, budgets, class_seeds in ((((5, 40), (6, 25)), None, None),
                                         (((5, 30), (5, 20), (6, 35)), [12, 20, 7], None),
                                         (((6, 18), (7, 33)), [9, 14], [123457, 99])):
        groups = _groups(m, layout)
        kw = dict(KW, seed=7, max_new_tokens=budgets if budgets else 16)
        if class_seeds:
            kw["class_seeds"] = class_seeds
        g.groups_stats = {"joint": 0, "separate": 0}
        out = g.generate_groups(groups, joint_sampling=True, **kw)
        assert g.groups_stats == {"joint": 1, "separate": 0}
        for gi, ((c, t), a) in enumerate(zip(groups, out)):
            seed = class_seeds[gi] if class_seeds else 7 + 7919 * gi
            nb = budgets[gi] if budgets else 16
            assert a.shape[1] <= nb and torch.equal(a, g.generate(c, t, **dict(KW, seed=seed, max_new_tokens=nb))), (layout, gi)
        ser = g.generate_groups(groups, **kw)
        assert g.groups_stats == {"joint": 1, "separate": 1}
        assert all(torch.equal(a, b) for a, b in zip(out, ser))
    del g.groups_stats


def test_generate_rolling_samples_with_job_seeds():
    """top_k 15 with job_seeds: more jobs than slots, ragged budgets -- every job equals generate(seed=job_seeds[j]), and the decode step
    stays full (admitted jobs join the live ones)"""
    m = tiny_model()
    g = m.gpt
    groups = _groups(m, ((5, 40), (6, 25)))
    jobs = [groups[0], groups[1], groups[1], groups[0], (groups[1][0][:5].contiguous(), groups[1][1][:5].contiguous())]
    jb, seeds = [20, 7, 13, 9, 16], [5, 6, 7, 8, 2 ** 40 + 3]
    g.rolling_stats = {}
    rolled = g.generate_rolling(jobs, group=5, job_seeds=seeds, **dict(KW, max_new_tokens=jb))
    st = g.rolling_stats
    del g.rolling_stats
    for (c, t), a, nb, s in zip(jobs, rolled, jb, seeds):
        assert a.shape[1] <= nb and torch.equal(a, g.generate(c, t, **dict(KW, seed=s, max_new_tokens=nb)))
    # 16 slots hold two or three of these jobs at once: the calls averaged more rows than any one job has
    assert st["calls"] > 0 and st["row_steps_issued"] / (st["calls"] * 5) > 6
    with pytest.raises(NotImplementedError):
        g.generate_rolling(jobs, **dict(KW, max_new_tokens=jb))
    with pytest.raises(ValueError):
        g.generate_rolling(jobs, job_seeds=seeds[:2], **dict(KW, max_new_tokens=jb))


def test_convert_offline_rolling_samples_like_the_waves():
    """convert_offline(rolling=True, joint_sampling=True) at the reference's sampling settings takes the rolling path and returns the
    wave path's tokens; without joint_sampling a sampled run keeps the waves"""
    from genvc_amd.parallel_offline import convert_offline
    m = tiny_model()
    sr = m.content_sample_rate
    wavs = [synth.synth_audio(400 + i, "src", int(n * sr)) for i, n in enumerate((2.5, 2.5, 2.0, 1.5, 2.5))]
    ref = synth.synth_audio(401, "ref", 72000)
    kw = dict(KW, seed=3, max_new_tokens=12, seg_len=1.0, micro_batch=3)
    waves = convert_offline(m, wavs, ref, **kw)
    m.gpt.rolling_stats = {}
    rolled = convert_offline(m, wavs, ref, rolling=True, joint_sampling=True, **kw)
    st = dict(m.gpt.rolling_stats)
    assert st.get("calls", 0) > 0
    assert rolled.shape == waves.shape and torch.equal(rolled, waves)
    m.gpt.rolling_stats = {}
    again = convert_offline(m, wavs, ref, rolling=True, **kw)
    assert m.gpt.rolling_stats == {} and torch.equal(again, waves)
    del m.gpt.rolling_stats


def test_stream_sessions_per_session_sampling():
    """StreamSessions(per_session_sampling=True): sessions with top_k 1, 15 and 50 opened and fed at different times each get the tokens
    and waveform of their solo synthesize_utt_streaming with the model config set to their settings; a session with seed 5 draws the
    same tokens beside different sessions; open(sampling=...) on a default scheduler raises"""
    from genvc_amd.inference.inference_utils import segments, synthesize_utt_streaming
    from genvc_amd.streaming import StreamSessions
    m = tiny_model(max_slots=8)
    cfg = m.config
    saved = dict(top_k=cfg.top_k, top_p=cfg.top_p, temperature=cfg.temperature, repetition_penalty=cfg.repetition_penalty)
    max_new = m.gpt.max_gen_mel_tokens
    m.gpt.max_gen_mel_tokens = 30
    try:
        refs = [synth.synth_audio(60 + i, "ref", 72000) for i in range(3)]
        srcs = [synth.synth_audio(80 + i, "src", n) for i, n in enumerate((32000, 16000, 40000))]
        segs = [list(segments(s, 16000, 5120)) for s in srcs]
        settings = [dict(top_k=1), dict(top_k=15, top_p=0.85, temperature=0.85, repetition_penalty=2.0),
                    dict(top_k=50, top_p=1.0, temperature=0.7, repetition_penalty=1.5)]

        def schedule(order, seeds):
            ss = StreamSessions(m, max_sessions=4, group=8, per_session_sampling=True)
            sids, wavs = {}, {}
            steps = 0
            first, second, third = order
            sids[first] = ss.open(refs[first], sampling=settings[first], seed=seeds[first])
            ss.push(sids[first], segs[first][0])
            while True:
                for sid, chunks in ss.step().items():
                    wavs.setdefault(sid, []).extend(chunks)
                steps += 1
                if steps == 1:
                    sids[second] = ss.open(refs[second], sampling=settings[second], seed=seeds[second])
                    for sg in segs[second]:
                        ss.push(sids[second], sg)
                    for sg in segs[first][1:]:
                        ss.push(sids[first], sg)
                if steps == 3:
                    sids[third] = ss.open(refs[third], sampling=settings[third], seed=seeds[third])
                    for sg in segs[third]:
                        ss.push(sids[third], sg)
                if steps > 3 and ss.idle():
                    break
                assert steps < 200
            return {i: (torch.cat(ss.close(sids[i]), 1)[0].cpu(), torch.cat(wavs[sids[i]], -1).cpu()) for i in order}

        got = schedule((0, 1, 2), (0, 0, 0))
        for i in range(3):
            for k, v in dict(saved, **settings[i]).items():
                setattr(cfg, k, v)
            solo = synthesize_utt_streaming(m, srcs[i], refs[i], seg_len=1.0, stream_chunk_size=8, verbose=False, return_details=True)
            for k, v in saved.items():
                setattr(cfg, k, v)
            assert torch.equal(got[i][0], torch.cat(solo["tokens"], 1)[0].cpu()), f"stream {i}: tokens differ from its solo run"
            assert got[i][1].shape == solo["wav"].shape
            np.testing.assert_allclose(got[i][1].numpy(), solo["wav"].cpu().numpy(), atol=2e-4)
        # session 1 with seed 5, scheduled with different neighbours and at a different time: the same tokens
        a = schedule((1, 0, 2), (0, 5, 0))[1][0]
        b = schedule((2, 1, 0), (0, 5, 0))[1][0]
        assert torch.equal(a, b) and not torch.equal(a, got[1][0])
        with pytest.raises(ValueError):
            StreamSessions(m, max_sessions=2).open(refs[0], sampling=dict(top_k=15))
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
        m.gpt.max_gen_mel_tokens = max_new
