"""CPU: the oracle restatement against the golden vectors produced by the reference's own
classes (oracle/make_golden.py).  These pin the oracle before any GPU test trusts it."""
import numpy as np
import pytest
import torch

from genvc_amd import config as gcfg
from genvc_amd import synth
from oracle import genvc_oracle as O

GREEDY = dict(gcfg.DEFAULT_SAMPLING, top_k=1)
_cache = {}


def weights(model_args, seed):
    key = (model_args["gpt_layers"], model_args["gpt_n_model_channels"], seed)
    if key not in _cache:
        dims = gcfg.gpt_dims(model_args)
        _cache.clear()
        _cache[key] = (dims, synth.make_weights(seed, synth.gpt_weight_spec(dims)))
    return _cache[key]


def inputs(g, dims):
    s, B, Tc = int(g["in_seed"]), int(g["B"]), int(g["Tc"])
    cond = synth.uniform(s, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (B, Tc), 256)
    return cond, codes


def check_gpt(g, model_args):
    dims, w = weights(model_args, int(g["seed"]))
    cond, codes = inputs(g, dims)
    prefix, fake = O.compute_embeddings(w, dims, cond, codes)
    assert np.array_equal(fake.numpy(), g["fake_ids"])
    assert abs(prefix.double().sum().item() - float(g["prefix_sum"])) < 1e-3
    np.testing.assert_allclose(prefix[:, -3:, :16].numpy(), g["prefix_slice"], atol=1e-6)
    n = g["tokens"].shape[1]
    toks, lats, logits = O.generate(w, dims, cond, codes, GREEDY, max_new=n)
    assert np.array_equal(toks.numpy(), g["tokens"])                       # bit-exact ids
    rows = g["logit_rows"]
    np.testing.assert_allclose(logits[rows].numpy(), g["logits"], atol=1e-4)
    np.testing.assert_allclose(lats[:, :, :32].numpy(), g["latents_slice"], atol=1e-4)
    # row 12: teacher-forced latent re-pass == decode-time latents
    gen = toks[0][toks[0] != dims["stop_audio_token"]].unsqueeze(0)
    rel = O.gpt_latents(w, dims, cond[:1], codes[:1], gen)
    assert rel.shape[1] == gen.shape[1]
    np.testing.assert_allclose(rel[:, :, :32].numpy(), g["relatents"], atol=1e-4)
    np.testing.assert_allclose(rel[:, :gen.shape[1]].numpy(), lats[:1, :gen.shape[1]].numpy(), atol=1e-4)


@pytest.mark.parametrize("name", ["gpt_tiny", "gpt_tiny_b1"])
def test_gpt_tiny_vs_reference(gold, name):
    check_gpt(gold(name), gcfg.TINY_MODEL_ARGS)


def test_gpt_eos_vs_reference(gold):
    g = gold("gpt_eos")
    dims, w = weights(gcfg.TINY_MODEL_ARGS, int(g["seed"]))
    w = dict(w)
    w["mel_head.bias"] = w["mel_head.bias"].clone()
    w["mel_head.bias"][1025] = float(g["stop_bias"])
    cond = synth.uniform(int(g["seed"]), "cond_latents", (2, 32, dims["d_model"]), 1.0)
    codes = synth.integers(int(g["seed"]), "content_codes", (2, 9), 256)
    toks, lats, _ = O.generate(w, dims, cond, codes, GREEDY, max_new=40)
    assert np.array_equal(toks.numpy(), g["tokens"])        # stops when every row hit 1025; pads after
    np.testing.assert_allclose(lats[:, :, :32].numpy(), g["latents_slice"], atol=1e-4)


def test_gpt_full_vs_reference(gold):
    check_gpt(gold("gpt_full"), gcfg.DEFAULT_MODEL_ARGS)


def test_perceiver_vs_reference(gold):
    g = gold("perceiver")
    seed = int(g["seed"])
    for tag, margs, wseed in (("tiny", gcfg.TINY_MODEL_ARGS, 3), ("full", gcfg.DEFAULT_MODEL_ARGS, 1)):
        dims = gcfg.gpt_dims(margs)
        w = synth.make_weights(wseed, synth.perceiver_weight_spec(dims["d_model"], prefix="conditioning_perceiver."))
        for B, Fr in ((1, 282), (2, 563)):
            mel = synth.uniform(seed, f"mel_{B}_{Fr}", (B, 80, Fr), 1.0)
            y = O.get_style_emb(w, mel)
            np.testing.assert_allclose(y.numpy(), g[f"{tag}_{B}_{Fr}"], atol=2e-5)


def test_dvae_vs_reference(gold):
    g = gold("dvae")
    seed = int(g["seed"])
    for tag, c in (("tiny", gcfg.TINY_CONTENT_DVAE), ("full", gcfg.DEFAULT_CONTENT_DVAE)):
        w = synth.make_weights(seed, synth.dvae_weight_spec(c))
        for B, T in ((1, 49), (2, 299), (1, 199), (1, 16)):
            feat = synth.uniform(seed, f"feat_{B}_{T}", (B, c["num_channels"], T), 1.0)
            codes = O.dvae_get_codebook_indices(w, feat)
            assert codes.shape == g[f"{tag}_codes_{B}_{T}"].shape            # 49->13, 299->75, 199->50
            assert np.array_equal(codes.numpy(), g[f"{tag}_codes_{B}_{T}"])
            enc = O.dvae_encode(w, feat)
            np.testing.assert_allclose(enc[:, :, :16].numpy(), g[f"{tag}_enc_{B}_{T}"], atol=1e-5)


def test_sampler_processors_vs_hf(gold):
    g = gold("sampler")
    logits = synth.uniform(int(g["seed"]), "logits", (4, 1026), 2.0)
    ids = torch.from_numpy(g["ids"])
    for k, p in ((1, 0.85), (15, 0.85), (50, 0.85), (15, 1.0), (1026, 0.5)):
        s = O.process_logits(logits, ids, 2.0, 0.85, k, p)
        ref = g[f"scores_k{k}_p{int(p * 100)}"]
        assert np.array_equal(np.isinf(s.numpy()), np.isinf(ref))
        m = ~np.isinf(ref)
        np.testing.assert_allclose(s.numpy()[m], ref[m], rtol=1e-6)
    # top_k=1 leaves exactly one candidate = argmax of the penalised logits
    s = O.process_logits(logits, ids, 2.0, 0.85, 1, 0.85)
    assert (torch.isfinite(s).sum(-1) == 1).all()


def test_mel_fp32_vs_float64_dft():
    """mel is 'parity unpinned' (torchaudio absent): cross-check the fp32 restatement against an
    independent float64 direct-DFT formulation, within the north_star tolerance 1e-4."""
    from genvc_amd.utils import DEFAULT_MEL_NORM_FILE
    mel_norms = torch.from_numpy(np.load(DEFAULT_MEL_NORM_FILE))
    wav = synth.synth_audio(21, "ref3s", 72000)
    m32 = O.mel_spectrogram(wav, mel_norms)
    assert m32.shape == (1, 80, 282)
    m64 = O.mel_spectrogram_dft64(wav.numpy(), mel_norms.numpy())
    np.testing.assert_allclose(m32.numpy(), m64, atol=1e-4)
    for T, Fr in ((144000, 563), (96000, 376), (98835, 387)):
        assert O.mel_spectrogram(synth.synth_audio(1, "x", T), mel_norms).shape[-1] == Fr


def test_segmentation_and_chunks():
    assert O.segment_source(160000, 6.0) == [(0, 96000, 96000), (96000, 160000, 64000)]
    assert O.segment_source(160000, 1.0)[-1] == (144000, 160000, 16000)
    assert O.segment_source(97000, 6.0)[-1] == (96000, 97000, 5120)          # padded to 0.32 s
    w1 = torch.arange(8192, dtype=torch.float32)
    c1, ov = O.handle_chunks(w1, None)
    assert c1.shape[0] == 7168 and ov.shape[0] == 1024
    c2, ov2 = O.handle_chunks(w1 + 1.0, ov)
    assert c2.shape[0] == 7168
    assert abs(float(c2[0]) - float(ov[0])) < 1e-6                            # fade starts at the old tail


def test_handle_chunks_vs_reference(gold):
    """the restated cross-fade against the reference's own handle_chunks (oracle/make_golden.py:make_handle_chunks):
    first chunk, cross-fades, a short group, the 1-token raw-tail branch and the un-faded chunk that follows it"""
    g = gold("handle_chunks")
    ov = None
    for i, n in enumerate(g["lens"]):
        wav = synth.uniform(int(g["seed"]), f"chunk{i}", (int(n),), 0.5)
        chunk, ov = O.handle_chunks(wav, ov)
        np.testing.assert_allclose(chunk.numpy(), g[f"chunk{i}"], rtol=0, atol=1e-7)
        assert (ov is not None) == bool(g[f"has_overlap{i}"])
        if ov is not None:
            np.testing.assert_array_equal(ov.numpy(), g[f"overlap{i}"])


def test_hifigan_vs_reference(gold):
    g = gold("hifigan")
    seed = int(g["seed"])
    for tag, c in (("tiny", gcfg.TINY_VOCODER), ("full", gcfg.DEFAULT_VOCODER)):
        w = synth.make_weights(seed, synth.hifigan_weight_spec(c))
        for B, n in ((1, 8), (2, 3), (1, 1)):
            lat = synth.uniform(seed, f"lat_{B}_{n}", (B, n, c["input_feat_dim"]), 1.0)
            wav = O.vocode_latents(w, c, lat)
            assert wav.shape == (B, 1, n * 4 * 256)
            np.testing.assert_allclose(wav.numpy(), g[f"{tag}_wav_{B}_{n}"], atol=2e-5)


def test_hubert_restatement_vs_hf(gold):
    """ContentVec / HuBERT-base forward (fairseq absent): restatement pinned to HuggingFace's HubertModel"""
    g = gold("hubert")
    seed = int(g["seed"])
    for tag, c in (("tiny", gcfg.TINY_HUBERT), ("full", gcfg.DEFAULT_HUBERT)):
        w = synth.make_weights(seed, synth.hubert_weight_spec(c))
        for B, T in ((1, 16000), (2, 5120), (1, 24581)):
            wav = torch.cat([synth.synth_audio(seed + b, f"wav{T}", T) for b in range(B)], 0)
            feat = O.hubert_extract_features(w, c, wav)
            ref = g[f"{tag}_feat_{B}_{T}"]
            assert feat.shape[:2] == ref.shape[:2] and feat.shape[-1] == 256
            np.testing.assert_allclose(feat.numpy()[:, :, :ref.shape[-1]], ref, atol=2e-4)


def test_hubert_padding_mask_semantics():
    """content_processor.py:24 + fairseq forward_padding_mask: trailing T % F samples dropped, a frame is padding when its
    whole chunk is zero; an input without an all-zero chunk takes the mask-free path bit for bit"""
    from genvc_amd import config as gcfg
    c = gcfg.TINY_HUBERT
    w = synth.make_weights(23, synth.hubert_weight_spec(c), device="cpu")
    tail = torch.zeros(1, 5120)
    tail[:, :2000] = synth.synth_audio(41, "tail", 2000)
    pm = O.hubert_frame_padding_mask(tail, 15)                          # chunk = 341 samples, 5 dropped
    assert pm.int().tolist() == [[0] * 6 + [1] * 9]                     # frame 5 holds samples 1705..2045: 295 of them real
    a = O.hubert_extract_features(w, c, tail)
    assert bool(torch.isfinite(a).all())
    assert float((a - O.hubert_extract_features(w, c, tail, padding_mask=False)).abs().max()) > 1e-2
    sparse = synth.synth_audio(43, "sp", 16000).clone()
    sparse[:, ::7] = 0.0
    assert not bool(O.hubert_frame_padding_mask(sparse, 49).any())
    assert torch.equal(O.hubert_extract_features(w, c, sparse), O.hubert_extract_features(w, c, sparse, padding_mask=False))


@pytest.mark.parametrize("orig,new", [(96000, 16000), (96000, 24000), (22050, 16000), (16000, 24000)])
def test_resampler_restatement_on_band_limited_signals(orig, new):
    """row f2 (torchaudio absent: parity unpinned against torchaudio itself): the float64 restatement of its sinc_interp_hann
    recipe reproduces a band-limited signal sampled at the new rate (interior, filter ripple), agrees with
    scipy.signal.resample_poly -- another low-pass design -- to the two filters' ripple, has torchaudio's output length and is linear
    (the product has no CPU resampler: genvc_amd/audio.py resamples on the HIP kernel, which tests/test_gpu_frontend.py checks against this oracle)"""
    import math
    from scipy.signal import resample_poly
    T = 6000 * orig // 16000
    t_in = np.arange(T) / orig
    freqs, amps = [220.0, 1333.0, 0.35 * min(orig, new) / 2], [0.5, 0.3, 0.2]
    x = sum(a * np.sin(2 * np.pi * f * t_in + 0.3 * i) for i, (f, a) in enumerate(zip(freqs, amps)))
    y = O.resample(torch.from_numpy(x[None].astype(np.float32)), orig, new).numpy()[0].astype(np.float64)
    n_out = int(math.ceil(new * T / orig))
    assert y.shape[0] == n_out
    t_out = np.arange(n_out) / new
    exact = sum(a * np.sin(2 * np.pi * f * t_out + 0.3 * i) for i, (f, a) in enumerate(zip(freqs, amps)))
    edge = 64
    assert np.abs(y[edge:-edge] - exact[edge:-edge]).max() < 2e-3
    g = math.gcd(orig, new)
    sp = resample_poly(x, new // g, orig // g)
    m = min(len(sp), n_out)
    assert np.abs(y[edge:m - edge] - sp[edge:m - edge]).max() < 5e-3
    # linearity
    x2 = synth.synth_audio(3, "rs", T)
    a = O.resample(x2, orig, new)
    np.testing.assert_allclose(O.resample(2.5 * x2, orig, new).numpy(), 2.5 * a.numpy(), atol=1e-6)


def test_streaming_chain_full_size_vs_reference_classes(gold):
    """the ORACLE driven through the streaming harness at GenVC_small size (tests/chain_oracle.py: what the GPU test of the headline
    chain compares with) against the same chain composed from the REFERENCE's own classes (oracle/make_golden.py:make_chain: reference
    Perceiver / DVAE / GPT / HiFi-GAN / handle_chunks, HuggingFace HubertModel for ContentVec): codes and tokens equal, latents and the
    cross-faded waveform within float rounding.  Pins the composition -- segmentation, 24-token budget, groups of 8, x4 interpolation,
    cross-fade -- and not only the stages."""
    from chain_oracle import streaming_chain, synthetic_bundle
    g = gold("chain_full")
    cfg = gcfg.default_config()
    W = synthetic_bundle(cfg, int(g["seed"]), int(g["n_steps"]))
    src = synth.synth_audio(int(g["src_seed"]), "src", 48000)
    ref = synth.synth_audio(int(g["ref_seed"]), "ref", 72000)
    ex = streaming_chain(W, src, ref, 1.0, int(g["group"]))
    assert float(g["margins"].min()) >= 2e-3 and ex["token_margin"] >= 2e-3          # margin-screened source seed (both sides)
    assert np.array_equal(torch.cat(ex["codes"], 0).numpy(), g["codes"])
    assert np.array_equal(torch.cat(ex["tokens"], 1).numpy(), g["tokens"])
    np.testing.assert_allclose(ex["cond"].numpy()[:, :, :16], g["cond_slice"], atol=5e-5)
    np.testing.assert_allclose(torch.cat(ex["latents"], 1).numpy()[:, :, :32], g["latents_slice"], atol=1e-4)
    wav = ex["wav"].numpy()
    assert wav.shape[0] == int(g["wav_len"])
    np.testing.assert_allclose(wav[:4096], g["wav_head"], atol=1e-4)
    np.testing.assert_allclose(wav[::16], g["wav_stride16"], atol=1e-4)


def test_generation_loop_vs_the_references_own_sample_stream(gold):
    """tests/golden/stream_loop.npz holds what `NewGenerationMixin.sample_stream` ITSELF (reference layers/stream_generator.py:645-881,
    imported with four stand-in names and called through the reference's GPT.get_generator, oracle/make_golden.py:make_stream_loop) yields:
    (a) three rows ending at three different steps -- finished rows yield the pad, the loop ends with the last row, the EOS-step pair is
    yielded; (b) a run that ends on max_length; (c) GPT.generate (gpt.py:594-608) for the inputs of (b).  O.generate must yield the same."""
    g = gold("stream_loop")
    seed = int(g["seed"])
    dims, w = weights(gcfg.TINY_MODEL_ARGS, seed)
    w = dict(w)
    w["mel_head.bias"] = w["mel_head.bias"].clone()
    w["mel_head.bias"][1025] = float(g["eos_bias"])
    s = int(g["eos_in_seed"])
    cond = synth.uniform(s, "cond_latents", (3, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (3, 11), 256)
    toks, lats, _ = O.generate(w, dims, cond, codes, GREEDY)
    assert len(set(g["eos_ends"].tolist())) == 3                            # ragged: every row stops at its own step
    assert toks.shape[1] == g["eos_tokens"].shape[1] == int(g["eos_ends"].max()) + 1
    assert np.array_equal(toks.numpy(), g["eos_tokens"])
    for b, e in enumerate(g["eos_ends"]):                                   # latents of live rows (finished rows keep running on pads)
        np.testing.assert_allclose(lats[b, :e + 1, :32].numpy(), g["eos_latents_slice"][b, :e + 1], atol=1e-4)
        assert (g["eos_tokens"][b, e:] == 1025).all()
    w["mel_head.bias"][1025] = 0.0
    s = int(g["max_in_seed"])
    cond = synth.uniform(s, "cond_latents", (2, 32, dims["d_model"]), 1.0)
    codes = synth.integers(s, "content_codes", (2, 13), 256)
    n = int(g["max_new"])
    dims_short = dict(dims, max_gen_mel_tokens=n)
    toks, lats, _ = O.generate(w, dims_short, cond, codes, GREEDY)          # no max_new argument: the cap comes from the model's dims
    assert toks.shape[1] == n and float(g["max_margins"].min()) > 2e-3
    assert np.array_equal(toks.numpy(), g["max_tokens"]) and np.array_equal(toks.numpy(), g["generate_tokens"])
    np.testing.assert_allclose(lats[:, :, :32].numpy(), g["max_latents_slice"], atol=1e-4)


def _harness_bundle(tag, g, case):
    from chain_oracle import synthetic_bundle
    cfg = gcfg.default_config(tiny=tag == "tiny")
    W = synthetic_bundle(cfg, int(g["seed"]), int(g["max_new"]))
    if float(g[case + "_stop_bias"]) >= 0:
        W["gpt"] = dict(W["gpt"])
        W["gpt"]["mel_head.bias"] = W["gpt"]["mel_head.bias"].clone()
        W["gpt"]["mel_head.bias"][1025] = float(g[case + "_stop_bias"])
    src = synth.synth_audio(int(g[case + "_src_seed"]), "src", 35200)
    ref = synth.synth_audio(100, "ref", 72000)
    return W, src, ref


def check_harness_result(g, case, st, ns, atol_lat, atol_wav):
    """st / ns: dict(tokens=[...], latents=[...], wav) of the streaming run and dict(latents, wav) of the non-streaming one"""
    p = case + "_"
    assert [int(t.shape[1]) for t in st["tokens"]] == g[p + "groups"].tolist()                  # group boundaries, short tails, EOS pairs
    assert np.array_equal(torch.cat(st["tokens"], 1).cpu().numpy().reshape(-1), g[p + "tokens"])
    np.testing.assert_allclose(torch.cat(st["latents"], 1).cpu().numpy()[0, :, :32], g[p + "latents_slice"], atol=atol_lat)
    wav = st["wav"].cpu().numpy()
    assert wav.shape[0] == int(g[p + "wav_len"])
    np.testing.assert_allclose(wav[:4096], g[p + "wav_head"], atol=atol_wav)
    np.testing.assert_allclose(wav[::8], g[p + "wav_stride8"], atol=atol_wav)
    assert int(ns["latents"].shape[1]) == int(g[p + "ns_latent_rows"].sum())                  # stop tokens stripped (inference_utils.py:68)
    wn = ns["wav"].cpu().numpy()
    assert wn.shape[0] == int(g[p + "ns_wav_len"])
    np.testing.assert_allclose(wn[:4096], g[p + "ns_wav_head"], atol=atol_wav)
    np.testing.assert_allclose(wn[::8], g[p + "ns_wav_stride8"], atol=atol_wav)


@pytest.mark.parametrize("tag,case", [("tiny", "max"), ("tiny", "eos"), ("full", "max")])
def test_harness_vs_the_references_own_functions(gold, tag, case):
    """tests/golden/harness_*.npz: the reference's UNCHANGED synthesize_utt_streaming(seg_len=1.0, stream_chunk_size=8) and synthesize_utt
    (inference/inference_utils.py:135-217, :23-89) called on a model object made of the reference's own classes with the reference's
    sample_stream behind get_generator / generate (oracle/make_golden.py:make_harness).  2.2 s source: two 1 s segments and a 0.2 s tail
    zero-padded to 0.32 s (:43-50).  The oracle's harness restatement must reproduce tokens, group boundaries, latents and both waveforms."""
    g = gold("harness_" + tag)
    W, src, ref = _harness_bundle(tag, g, case)
    assert float(g[case + "_margin"]) > 2e-3 and int(g[case + "_masked_segments"]) == 1
    st = O.synthesize_utt_streaming(W, src, ref, seg_len=1.0, stream_chunk_size=8)
    ns = O.synthesize_utt(W, src, ref, seg_len=1.0)
    check_harness_result(g, case, st, ns, 1e-4, 1e-4)


def test_third_party_pins_when_present(gold):
    """oracle/pin_third_party.py writes mel.npz / resample.npz (torchaudio) and hubert_fairseq.npz (fairseq) where those wheels exist;
    this container has neither, so the files are absent and the three stages stay pinned to their published algorithms.
    Whoever runs the recipe gets the checks for free."""
    import os
    from conftest import GOLD
    from genvc_amd.utils import DEFAULT_MEL_NORM_FILE, load_mel_norms
    ran = 0
    if os.path.exists(os.path.join(GOLD, "mel.npz")):
        g = gold("mel")
        norms = torch.from_numpy(load_mel_norms(DEFAULT_MEL_NORM_FILE))
        np.testing.assert_allclose(O.mel_spectrogram(synth.synth_audio(100, "ref", 72000), norms).numpy(), g["mel"], atol=1e-4)
        ran += 1
    if os.path.exists(os.path.join(GOLD, "resample.npz")):
        g = gold("resample")
        for o, n in ((96000, 16000), (96000, 24000), (22050, 16000), (16000, 24000)):
            x = synth.synth_audio(3, "rs", 6000 * o // 16000)
            np.testing.assert_allclose(O.resample(x, o, n).numpy(), g[f"y_{o}_{n}"], atol=2e-5)
        ran += 1
    if os.path.exists(os.path.join(GOLD, "hubert_fairseq.npz")):
        g = gold("hubert_fairseq")
        w = synth.make_weights(17, synth.hubert_weight_spec(gcfg.DEFAULT_HUBERT))
        tail = torch.zeros(1, 5120)
        tail[:, :2000] = synth.synth_audio(41, "tail", 2000)
        hole = synth.synth_audio(43, "hole", 16000).clone()
        hole[:, 6000:9000] = 0.0
        for name, wav in (("plain", synth.synth_audio(17, "wav16000", 16000)), ("zero_tail", tail), ("interior_silence", hole)):
            np.testing.assert_allclose(O.hubert_extract_features(w, gcfg.DEFAULT_HUBERT, wav).numpy(), g[name], atol=2e-4)
        ran += 1
    if ran == 0:
        pytest.skip("torchaudio / fairseq fixtures absent: mel, resampler and ContentVec stay pinned to their published algorithms")
