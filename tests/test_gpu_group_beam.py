"""GPU: group (diverse) beam search (include/genvc_hip.h: gvc_beam_groups, gvc_group_beam_select, gvc_gpt_group_beam_generate) against
the CPU restatement (tests/group_beam_oracle.py) and tests/golden/group_beam.npz (scripts/make_group_beam_golden.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_oracle as BO                      # noqa: E402
import group_beam_oracle as GO                # noqa: E402
import nbest_oracle as NO                     # noqa: E402
from genvc_amd import config as gcfg          # noqa: E402
from genvc_amd import synth                   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOS, V = 1025, 1026
EOS_CYCLE = [9.0, 3.0, 5.0, 1.0, 7.0, 4.0]


def make_gpt(model_args, seed, stop_bias=None, max_slots=16):
    from genvc_amd.layers.gpt import GPT
    a = model_args
    g = GPT(layers=a["gpt_layers"], model_dim=a["gpt_n_model_channels"], heads=a["gpt_n_heads"],
            max_text_tokens=a["gpt_max_text_tokens"], max_mel_tokens=a["gpt_max_audio_tokens"],
            max_prompt_tokens=a["gpt_max_prompt_tokens"], number_text_tokens=a["gpt_number_text_tokens"],
            start_text_token=a["gpt_start_text_token"], stop_text_token=a["gpt_stop_text_token"],
            num_audio_tokens=a["gpt_num_audio_tokens"], start_audio_token=a["gpt_start_audio_token"],
            stop_audio_token=a["gpt_stop_audio_token"], code_stride_len=a["gpt_code_stride_len"])
    dims = gcfg.gpt_dims(a)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][EOS] = float(stop_bias)
    g.load_state_dict(w, strict=False)
    g.to(DEV)
    g.init_gpt_for_inference(max_slots=max_slots)
    return g, w, dims


def _group_set(beam, b, g):
    S = beam.S
    n = int(beam.group_count[b, g])
    hs, hl, ht = beam.hyp_score[b, g * S:].cpu(), beam.hyp_len[b, g * S:].cpu(), beam.hyp_tok[b, g * S:].cpu()
    return sorted((float(hs[i]), ht[i, :int(hl[i])].tolist()) for i in range(n))


# ---- 1. one select step against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,G", [(1, 2, 2), (3, 4, 2), (2, 6, 3), (1, 8, 8), (2, 16, 4), (1, 16, 16)])
@pytest.mark.parametrize("mode", ["4.33", "generated"])
def test_group_select_matches_restatement(B, K, G, mode, monkeypatch):
    from genvc_amd.engine import GroupBeamSearch, group_beam_select
    n0, max_new, rep, S = 7, 12, 2.0, K // G
    # (the plain formula's stream for (1, 2, 2) never puts eos at rank 1 of a single row's top 2: the final assertion names it)
    gen_ = torch.Generator().manual_seed(1000 * B + 10 * K + G + (200000 if (B, K, G) == (1, 2, 2) else 0))
    fake = torch.randint(0, 1024, (B, n0), generator=gen_)
    fake[:, -1] = 1024
    ranks_seen = set()
    plain_step = NO.select_step

    def watched(s, scores, gen, hyps, done, t, n0_, K_, V_, eos, *a):
        acc = (s + scores[:, None]).view(len(hyps), -1)
        for b in range(len(hyps)):
            if not done[b]:
                top = torch.topk(acc[b], 2 * K_)[1]
                ranks_seen.update(int(r >= K_) for r, i in enumerate(top.tolist()) if i % V_ == eos)
        return plain_step(s, scores, gen, hyps, done, t, n0_, K_, V_, eos, *a)
    monkeypatch.setattr(GO.NO, "select_step", watched)
    for lp, lam in ((0.5, 0.5), (1.0, 5.0), (2.0, 0.5), (0.5, 5.0), (1.0, 0.5), (2.0, 5.0)):
        beam = GroupBeamSearch(fake.to(DEV), K, G, lam, max_new, EOS, V, lp, rep, mode)
        slots = torch.arange(B * K, device=DEV, dtype=torch.int32)
        scores = beam.scores.cpu().clone()
        assert torch.equal(scores, GO.start_scores(B, K, G))
        gen = [[] for _ in range(B * K)]
        hyps = [[BO.Hyps(S) for _ in range(G)] for _ in range(B)]
        done = [[False] * G for _ in range(B)]
        ids = fake.repeat_interleave(K, 0)
        for t in range(max_new - 1):
            logits = torch.randn(B * K, V, generator=gen_) * 3.0
            logits[:, EOS] += EOS_CYCLE[t % 6]                        # eos candidates above and below rank S
            was_done = [list(d) for d in done]
            ls = torch.log_softmax(logits.float(), dim=-1)
            tok, par, scores, gen, gap = GO.select_step(ls, ids, scores, gen, hyps, done, t, n0, K, G, lam, V, EOS, lp, rep, mode)
            assert gap > 1e-5, f"near-tie in the random case (gap {gap:.2e}): pick another seed"
            old_slots = slots.cpu().numpy().copy()
            group_beam_select(beam, logits.to(DEV).contiguous(), slots, t)
            beam.steps = t + 1
            torch.cuda.synchronize()
            assert np.array_equal(beam.tokens.cpu().numpy(), tok.numpy()), (t, lp, lam)
            assert np.array_equal(beam.parents.cpu().numpy(), par.numpy()), (t, lp, lam)
            torch.testing.assert_close(beam.scores.cpu(), scores.float(), rtol=1e-5, atol=1e-4)
            assert beam.group_done.cpu().tolist() == [[int(x) for x in d] for d in done], (t, lp, lam)
            assert beam.done.cpu().tolist() == [int(all(d)) for d in done], (t, lp, lam)
            for b in range(B):
                for g in range(G):
                    if was_done[b][g]:
                        continue
                    dev_h = _group_set(beam, b, g)
                    ref_h = sorted((sc, tk) for sc, tk in hyps[b][g].items)
                    assert [h[1] for h in dev_h] == [h[1] for h in ref_h], (t, lp, lam, b, g)
                    np.testing.assert_allclose([h[0] for h in dev_h], [h[0] for h in ref_h], rtol=1e-5, atol=1e-6)
                    worst = hyps[b][g].worst
                    assert abs(float(beam.group_worst[b, g]) - (worst if hyps[b][g].items else 1e9)) <= 1e-5 * max(1.0, abs(worst))
            # the slot permutation runs inside each group: slots stay a permutation, group by group, with at most K - G copies per item
            sl = slots.cpu().numpy()
            assert sorted(sl.tolist()) == list(range(B * K))
            for b in range(B):
                for g in range(G):
                    r = slice(b * K + g * S, b * K + (g + 1) * S)
                    assert sorted(sl[r].tolist()) == sorted(old_slots[r].tolist())
                    assert set((par[r] // S).tolist()) == {g}
                assert 0 <= int(beam.n_copies[b]) <= K - G
                if all(was_done[b]):
                    assert int(beam.n_copies[b]) == 0
            src = (torch.arange(B).repeat_interleave(K) * K + par).long()
            ids = torch.cat([ids[src], tok[:, None]], 1)
            assert np.array_equal(beam.ids[(t + 1) & 1, :, :n0 + t + 1].cpu().numpy(), ids.numpy())
            if all(all(d) for d in done):
                break
    assert ranks_seen == {0, 1}, f"eos candidates seen only at {'rank < S' if 0 in ranks_seen else 'rank >= S'}"


# ---- 2. G = 1 through the group entry is the plain select, bit for bit -------------------------------------------------------------
@pytest.mark.parametrize("B,K,procs", [(3, 4, False), (2, 16, False), (2, 5, True)])
def test_one_group_through_the_group_entry_is_bit_identical(B, K, procs):
    from genvc_amd.engine import BeamSearch, GroupBeamSearch, beam_select, group_beam_select, logits_processors
    n0, max_new = 7, 12
    gen_ = torch.Generator().manual_seed(77 + K)
    fake = torch.randint(0, 1024, (B, n0), generator=gen_)
    proc = logits_processors(dict(min_new_tokens=3, no_repeat_ngram_size=2), n0, V, sampling=False) if procs else None
    for mode, lp, early in (("4.33", 1.0, False), ("generated", 0.5, "never"), ("generated", 2.0, True)):
        a = BeamSearch(fake.to(DEV), K, max_new, EOS, V, lp, 2.0, mode, proc=proc, early_stopping=early)
        b = GroupBeamSearch(fake.to(DEV), K, 1, 0.0, max_new, EOS, V, lp, 2.0, mode, proc=proc, early_stopping=early)
        sa = torch.arange(B * K, device=DEV, dtype=torch.int32)
        sb = sa.clone()
        for t in range(max_new - 1):
            logits = (torch.randn(B * K, V, generator=gen_) * 3.0)
            logits[:, EOS] += EOS_CYCLE[t % 6]
            logits = logits.to(DEV).contiguous()
            beam_select(a, logits, sa, t)
            group_beam_select(b, logits, sb, t)
            a.steps = b.steps = t + 1
            torch.cuda.synchronize()
            for name in ("ids", "scores", "tokens", "parents", "done", "hyp_score", "hyp_len", "hyp_tok", "hyp_count", "hyp_worst",
                         "copies", "n_copies"):
                assert torch.equal(getattr(a, name), getattr(b, name)), (name, t, mode)
            assert torch.equal(sa, sb)
            assert torch.equal(b.group_done.view(-1), a.done) and torch.equal(b.group_count.view(-1), a.hyp_count)
            assert torch.equal(b.group_worst.view(-1), a.hyp_worst)


# ---- 3. slot permutation, fan-out and KV span copies -----------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,G,steps", [(2, 4, 2, 11), (1, 6, 3, 17)])
def test_group_beam_slots_hold_the_kv_a_replay_writes(B, K, G, steps):
    from genvc_amd.engine import GroupBeamSearch
    g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, 29)
    eng = g.engine
    cond = synth.uniform(2950, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
    codes = synth.integers(2950, "content_codes", (B, 9), 256).to(DEV)
    fake = g.compute_embeddings(cond, codes)
    prefix = g._prefix
    n0 = int(fake.shape[1])
    slots = torch.arange(B * K, device=DEV, dtype=torch.int32)
    eng.prefill(slots[::K].contiguous(), prefix, want_outputs=False)
    beam = GroupBeamSearch(fake, K, G, 1.0, 40, EOS, V, 1.0, 2.0, "4.33")
    eng.group_beam_generate(slots, beam, 1)                # step 0: the prefix was fanned out, every group's children come from its beam 0
    assert int(beam.n_copies[0]) == K - G
    assert beam.parents.view(B, K).cpu().tolist() == [[(k // (K // G)) * (K // G) for k in range(K)]] * B
    eng.group_beam_generate(slots, beam, steps - 1)
    torch.cuda.synchronize()
    eng.health()
    assert sorted(slots.cpu().tolist()) == list(range(B * K))
    T = beam.steps
    toks = beam.ids[T & 1, :, n0:n0 + T].clone()
    spare = torch.tensor([B * K], device=DEV, dtype=torch.int32)
    probe = torch.full((1,), 7, device=DEV, dtype=torch.int32)
    for r in range(B * K):
        b = r // K
        eng.reset(spare)
        eng.prefill(spare, prefix[b:b + 1].contiguous(), want_outputs=False)
        for j in range(T):
            eng.decode_step(spare, toks[r, j:j + 1].contiguous())
        ref, _ = eng.decode_step(spare, probe)
        got, _ = eng.decode_step(slots[r:r + 1].contiguous(), probe)
        torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4)


# ---- 4. GPT.generate against the fixture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_step", ["1", "0"])
def test_generate_reproduces_the_fixture(rows_step, monkeypatch):
    monkeypatch.setenv("GVC_PERSIST_ROWS", rows_step)
    gold = dict(np.load(os.path.join(GOLDEN, "group_beam.npz")))
    made = {}
    for tag in ("a0", "a1", "a2", "a3", "b0", "b1", "c0", "c1", "d"):
        full = bool(gold[f"{tag}_full"])
        key = (full, int(gold[f"{tag}_seed"]), float(gold[f"{tag}_stop_bias"]))
        if key not in made:
            for old in made.values():
                old[0].engine.close()
            made.clear()
            torch.cuda.empty_cache()
            made[key] = make_gpt(gcfg.DEFAULT_MODEL_ARGS if full else gcfg.TINY_MODEL_ARGS, key[1], stop_bias=key[2] if key[2] != 0.0 else None)
        g, _, dims = made[key]
        g.max_gen_mel_tokens = int(gold[f"{tag}_max_new"])
        B, K, G, Tc, s = (int(gold[f"{tag}_{n}"]) for n in ("B", "K", "G", "Tc", "in_seed"))
        cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
        codes = synth.integers(s, "content_codes", (B, Tc), 256).to(DEV)
        for i in range(int(gold[f"{tag}_n"])):
            p = f"{tag}_{i}_"
            assert float(gold[p + "min_gap"]) >= 1e-3 and float(gold[p + "order_gap"]) >= 1e-3       # the fixture's screens
            kw = dict(num_beams=K, num_beam_groups=G, diversity_penalty=float(gold[f"{tag}_lam"]), do_sample=False,
                      length_penalty=float(gold[p + "lp"]), repetition_penalty=float(gold[f"{tag}_rep"]),
                      beam_length_mode=str(gold[p + "mode"]), early_stopping=NO.EARLY[int(gold[p + "early"])], group=8,
                      **json.loads(str(gold[p + "proc"])))
            for N, sfx in ((K, ""), (1, "1")):
                ids = g.generate(cond, codes, num_return_sequences=N, **kw)
                assert ids.shape == gold[p + "ids" + sfx].shape and np.array_equal(ids.cpu().numpy(), gold[p + "ids" + sfx]), (tag, i, N)
                np.testing.assert_allclose(g.last_beam_scores.numpy(), gold[p + "scores" + sfx], rtol=1e-4, atol=1e-5)
                assert g.last_latents is None
    for old in made.values():
        old[0].engine.close()
    torch.cuda.empty_cache()


# ---- 5. warmed-up group calls do not allocate; plain beams are untouched -----------------------------------------------------------
def test_group_path_warm_and_plain_beams_unchanged():
    gold = dict(np.load(os.path.join(GOLDEN, "beam_search.npz")))
    for tag in ("a", "b"):
        assert not bool(gold[f"{tag}_full"])
        sb = float(gold[f"{tag}_stop_bias"])
        g, _, dims = make_gpt(gcfg.TINY_MODEL_ARGS, int(gold[f"{tag}_seed"]), stop_bias=sb if sb != 0.0 else None)
        eng = g.engine
        g.max_gen_mel_tokens = int(gold[f"{tag}_max_new"])
        B, K, Tc, s = int(gold[f"{tag}_B"]), int(gold[f"{tag}_K"]), int(gold[f"{tag}_Tc"]), int(gold[f"{tag}_in_seed"])
        cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0).to(DEV)
        codes = synth.integers(s, "content_codes", (B, Tc), 256).to(DEV)
        plain = dict(num_beams=K, do_sample=False, repetition_penalty=float(gold[f"{tag}_rep"]), beam_length_mode="generated", group=8)
        if tag == "a":
            assert K == 4
            n0 = 32 + Tc + 3
            eng.warmup_group_beam(B, K, 2, n0 + g.max_gen_mel_tokens)
            eng.warmup_beam(B, K, n0 + g.max_gen_mel_tokens)
            g.generate(cond, codes, length_penalty=1.0, **plain)
            base = eng.lazy_inits()
            g.generate(cond, codes, length_penalty=1.0, num_beam_groups=2, diversity_penalty=1.0, **plain)
            assert eng.lazy_inits() == base                   # the warmed group path neither allocates nor captures
        for i in range(int(gold[f"{tag}_n"])):
            if K % 2 == 0:                                    # a group call in between leaves nothing behind that a plain call sees
                g.generate(cond, codes, length_penalty=1.0, num_beam_groups=2, diversity_penalty=1.0, **plain)
            ids = g.generate(cond, codes, length_penalty=float(gold[f"{tag}_{i}_lp"]), **plain)
            assert np.array_equal(ids.cpu().numpy(), gold[f"{tag}_{i}_ids"]), (tag, i)
            np.testing.assert_allclose(g.last_beam_scores.numpy(), gold[f"{tag}_{i}_best_scores"], rtol=1e-4, atol=1e-5)
        g.engine.close()
        del g
        torch.cuda.empty_cache()


# ---- 6. GenVCModel.inference with groups -----------------------------------------------------------------------------------------
def test_model_inference_with_groups():
    from genvc_amd.inference.model_init import model_init_synthetic
    cfg = gcfg.default_config(tiny=True)
    m = model_init_synthetic(cfg, seed=1, device=DEV, max_slots=8)[0]
    m.gpt.max_gen_mel_tokens = 30
    src = synth.uniform(402, "src_wav", (1, 16000), 0.3).to(DEV)
    ref = synth.uniform(100, "ref_wav", (1, 24000 * 3), 0.3).to(DEV)
    cond = m.get_gpt_cond_latents(ref, 24000)
    kw = dict(do_sample=False, num_beams=4, num_beam_groups=2, diversity_penalty=1.0, num_return_sequences=4, repetition_penalty=2.0)
    wavs = m.inference(src, cond, **kw)
    feat = m.content_extractor.extract_content_features(src)
    codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
    rows = m.gpt.generate(cond, codes, **kw)
    assert isinstance(wavs, list) and len(wavs) == 4 and rows.shape[0] == 4
    assert m.last_beam_scores is not None and len(m.last_beam_scores) == 4
    assert len({tuple(r.tolist()) for r in rows}) == 4
    for j in range(4):
        n = int((rows[j] != EOS).sum())
        assert wavs[j].shape[-1] == n * 4 * 256
    one = m.inference(src, cond, **dict(kw, num_return_sequences=1))
    assert one.shape[-1] == wavs[0].shape[-1]
