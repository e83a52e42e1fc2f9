"""GPU parity of the front-end kernels: mel, Perceiver, content DVAE + VQ (through the C ABI)."""
import numpy as np
import pytest
import torch

from genvc_amd import config as gcfg
from genvc_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_mel_matches_oracle_within_1e4():
    from genvc_amd.engine import MelEngine
    from genvc_amd.utils import DEFAULT_MEL_NORM_FILE
    from oracle import genvc_oracle as O
    norms = np.load(DEFAULT_MEL_NORM_FILE)
    eng = MelEngine(norms)
    for T, frames in ((72000, 282), (144000, 563), (96000, 376), (98835, 387), (8000, 32)):
        wav = synth.synth_audio(21, f"ref{T}", T)
        wav = torch.cat([wav, synth.synth_audio(22, f"ref{T}", T, amplitude=0.5)], 0)
        got, fm = eng.forward(wav.to(DEV), frames_major=True)
        assert got.shape == (2, 80, frames)
        ref32 = O.mel_spectrogram(wav, torch.from_numpy(norms))
        ref64 = O.mel_spectrogram_dft64(wav.numpy(), norms)
        np.testing.assert_allclose(got.cpu().numpy(), ref64, atol=1e-4)      # north_star: mel within 1e-4
        np.testing.assert_allclose(got.cpu().numpy(), ref32.numpy(), atol=1e-4)
        assert torch.equal(fm.transpose(1, 2), got)


def test_perceiver_matches_reference(gold):
    from genvc_amd.engine import PerceiverEngine
    g = gold("perceiver")
    seed = int(g["seed"])
    for tag, margs, wseed in (("tiny", gcfg.TINY_MODEL_ARGS, 3), ("full", gcfg.DEFAULT_MODEL_ARGS, 1)):
        d = margs["gpt_n_model_channels"]
        w = synth.make_weights(wseed, synth.perceiver_weight_spec(d, prefix="conditioning_perceiver."), device=DEV)
        eng = PerceiverEngine(dim=d, depth=4, dim_context=80, num_latents=32, dim_head=64, heads=8, ff_mult=4,
                              max_batch=2, max_frames=600)
        eng.bind(w, prefix="conditioning_perceiver.")
        for B, Fr in ((1, 282), (2, 563)):
            mel = synth.uniform(seed, f"mel_{B}_{Fr}", (B, 80, Fr), 1.0).to(DEV)
            y = eng.forward(mel.permute(0, 2, 1).contiguous())          # [B,32,d]
            np.testing.assert_allclose(y.transpose(1, 2).cpu().numpy(), g[f"{tag}_{B}_{Fr}"], atol=5e-5)
        eng.close()


def test_dvae_codes_match_reference(gold):
    from genvc_amd.engine import DvaeEngine, vq_argmin
    g = gold("dvae")
    seed = int(g["seed"])
    n_safe = n_all = n_exempt_diff = 0
    for tag, c in (("tiny", gcfg.TINY_CONTENT_DVAE), ("full", gcfg.DEFAULT_CONTENT_DVAE)):
        w = synth.make_weights(seed, synth.dvae_weight_spec(c), device=DEV)
        eng = DvaeEngine(c, max_batch=2, max_frames=304)
        eng.bind(w)
        for B, T in ((1, 49), (2, 299), (1, 199), (1, 16)):
            feat = synth.uniform(seed, f"feat_{B}_{T}", (B, c["num_channels"], T), 1.0).to(DEV)
            codes, enc = eng.encode(feat, return_enc=True)
            ref = g[f"{tag}_codes_{B}_{T}"]
            assert codes.shape == ref.shape
            np.testing.assert_allclose(enc[:, :, :16].cpu().numpy(), g[f"{tag}_enc_{B}_{T}"], atol=2e-5)
            # bit-exact wherever the reference's own decision margin exceeds fp32 reassociation noise
            safe = g[f"{tag}_margin_{B}_{T}"] > 1e-4
            n_safe += int(safe.sum()); n_all += safe.size
            assert np.array_equal(codes.cpu().numpy()[safe], ref[safe])
            n_exempt_diff += int((codes.cpu().numpy()[~safe] != ref[~safe]).sum())
            # standalone VQ entry point on the same encoder output
            idx = vq_argmin(enc.reshape(-1, enc.shape[-1]).contiguous(), w["codebook.embed"])
            assert torch.equal(idx.view_as(codes), codes)
        eng.close()
    assert n_safe > 0.97 * n_all          # the margin screen excludes only a handful of frames
    # ... and how many of the exempt (near-tie) frames actually differ: the count is printed with `pytest -s` and bounded
    print(f"DVAE codes: {n_all} frames, {n_all - n_safe} with a reference margin <= 1e-4, {n_exempt_diff} of those differ")
    assert n_exempt_diff <= max(2, (n_all - n_safe) // 4)


@pytest.mark.parametrize("cfg", [
    dict(num_channels=256, hidden_dim=256, codebook_dim=256, num_resnet_blocks=2, kernel_size=3, num_layers=2),     # 1 / 1 / 2 channel slices
    dict(num_channels=512, hidden_dim=256, codebook_dim=128, num_resnet_blocks=1, kernel_size=5, num_layers=3),     # 5 taps, 3 stages, 4 slices
    dict(num_channels=256, hidden_dim=128, codebook_dim=64, num_resnet_blocks=2, kernel_size=3, num_layers=2),      # 128-channel stage: tiled GEMM only
], ids=["2slices", "5taps_3stages", "gemm_only"])
def test_dvae_other_configurations_match_oracle(cfg):
    """row a5 beyond the trained configuration: encoders of other shapes against the oracle (oracle/genvc_oracle.py dvae_encode, pinned to
    the reference class by tests/test_oracle.py); frame counts either side of the switch between the one-round-trip conv kernel
    (B x T <= 600) and the tiled GEMM, in an order that changes the buffer geometry between calls"""
    from genvc_amd.engine import DvaeEngine
    from oracle import genvc_oracle as O
    c = dict(gcfg.DEFAULT_CONTENT_DVAE, **cfg)
    w = synth.make_weights(31, synth.dvae_weight_spec(c))
    eng = DvaeEngine(c, max_batch=3, max_frames=400)
    eng.bind({k: v.to(DEV) for k, v in w.items()})
    for B, T in ((1, 49), (3, 350), (2, 17), (1, 333), (3, 49), (1, 49)):
        feat = synth.uniform(31, f"feat_{B}_{T}", (B, c["num_channels"], T), 1.0)
        ref = O.dvae_encode(w, feat)
        codes, enc = eng.encode(feat.to(DEV), return_enc=True)
        assert enc.shape == ref.shape
        np.testing.assert_allclose(enc.cpu().numpy(), ref.numpy(), atol=3e-5)
        # codes: equal wherever the oracle's own decision is not a near-tie
        flat = ref.reshape(-1, ref.shape[-1])
        dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ w["codebook.embed"] + w["codebook.embed"].pow(2).sum(0, keepdim=True)
        top2 = (-dist).topk(2, dim=1).values
        safe = ((top2[:, 0] - top2[:, 1]) > 1e-3).view(ref.shape[:-1]).numpy()
        exp = O.vq_indices(ref, w["codebook.embed"]).numpy()
        assert safe.mean() > 0.9 and np.array_equal(codes.cpu().numpy()[safe], exp[safe])
    eng.close()


def test_vq_first_index_wins_ties():
    from genvc_amd.engine import vq_argmin
    embed = synth.uniform(3, "e", (64, 32), 1.0).to(DEV)
    embed[:, 7] = embed[:, 20]                       # duplicate code: the lower index must win
    x = embed[:, [20, 5, 7]].t().contiguous()
    assert vq_argmin(x, embed).cpu().tolist() == [7, 5, 7]


def test_hifigan_matches_reference(gold):
    """row f1: HIP HiFi-GAN generator (latents -> x4 interpolation -> waveform) vs the reference's own class"""
    from genvc_amd.engine import HifiganEngine
    g = gold("hifigan")
    seed = int(g["seed"])
    for tag, c in (("tiny", gcfg.TINY_VOCODER), ("full", gcfg.DEFAULT_VOCODER)):
        w = synth.make_weights(seed, synth.hifigan_weight_spec(c), device=DEV)
        eng = HifiganEngine(c, max_batch=2, max_frames=64)
        eng.bind(w)
        for B, n in ((1, 8), (2, 3), (1, 1), (1, 8)):
            lat = synth.uniform(seed, f"lat_{B}_{n}", (B, n, c["input_feat_dim"]), 1.0).to(DEV)
            wav = eng.forward_latents(lat, 4)
            ref = g[f"{tag}_wav_{B}_{n}"]
            assert wav.shape == ref.shape
            np.testing.assert_allclose(wav.cpu().numpy(), ref, atol=1e-4)
            # reference-layout entry point: x [B,d,T] already interpolated
            mel = torch.nn.functional.interpolate(lat.transpose(1, 2), scale_factor=[4.0], mode="linear").contiguous()
            np.testing.assert_allclose(eng.forward(mel).cpu().numpy(), ref, atol=1e-4)
        eng.close()


@pytest.mark.parametrize("mode", ["0", "2"])
def test_hifigan_fallback_paths_match_reference(gold, monkeypatch, mode):
    """row f1: the paths behind GVC_VOCODER_SMALL_CONV -- 0: every conv on the tiled GEMM, one launch per conv, running ResBlock sum;
    2: ResBlock planes from the LDS conv kernel, added by k_sum_planes for a tiled-GEMM upsampling layer -- and the launch-per-call
    variants of the graph (GVC_VOCODER_GRAPH=0 / 2) against the same reference vectors as the default path"""
    from genvc_amd.engine import HifiganEngine
    g = gold("hifigan")
    seed = int(g["seed"])
    c = gcfg.DEFAULT_VOCODER
    w = synth.make_weights(seed, synth.hifigan_weight_spec(c), device=DEV)
    for graph in ("1", "0", "2"):
        monkeypatch.setenv("GVC_VOCODER_SMALL_CONV", mode if graph == "1" else "1")
        monkeypatch.setenv("GVC_VOCODER_GRAPH", graph)
        eng = HifiganEngine(c, max_batch=2, max_frames=64)
        eng.bind(w)
        for B, n in ((1, 8), (2, 3), (1, 8)):
            lat = synth.uniform(seed, f"lat_{B}_{n}", (B, n, c["input_feat_dim"]), 1.0).to(DEV)
            np.testing.assert_allclose(eng.forward_latents(lat, 4).cpu().numpy(), g[f"full_wav_{B}_{n}"], atol=1e-4)
        eng.close()


@pytest.mark.parametrize("cfg", [
    # other widths / rates / taps / dilations than the trained generator: every k_conv_lds instance, frame counts that are not whole
    # tiles, ResBlock counts that keep the launch-per-conv path, a stage narrower than the LDS kernel takes
    dict(input_feat_dim=512, upsample_initial_channel=512, resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3], [3, 5], [1, 7]],
         upsample_rates=[4, 4, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4]),
    dict(input_feat_dim=256, upsample_initial_channel=128, resblock_kernel_sizes=[5, 3, 9], resblock_dilation_sizes=[[2, 1], [1, 4], [3, 2]],
         upsample_rates=[8, 2], upsample_kernel_sizes=[16, 4]),
    dict(input_feat_dim=1024, upsample_initial_channel=256, resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 2], [2, 6]],
         upsample_rates=[8, 8, 4], upsample_kernel_sizes=[16, 16, 8]),
    dict(input_feat_dim=128, upsample_initial_channel=64, resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]],
         upsample_rates=[4, 4, 4], upsample_kernel_sizes=[8, 8, 8]),
], ids=["4stages_k11", "2stages", "2resblocks", "narrow"])
def test_hifigan_other_configurations_match_oracle(cfg):
    """row f1 beyond the trained configuration: generators of other shapes against the oracle's HiFi-GAN (oracle/genvc_oracle.py
    hifigan_forward, itself pinned to the reference class by tests/test_oracle.py)"""
    from genvc_amd.engine import HifiganEngine
    from oracle import genvc_oracle as O
    c = dict(gcfg.DEFAULT_VOCODER, **cfg)
    w = synth.make_weights(21, synth.hifigan_weight_spec(c))
    eng = HifiganEngine(c, max_batch=2, max_frames=64)
    eng.bind({k: v.to(DEV) for k, v in w.items()})
    for B, n in ((1, 5), (2, 9), (1, 16), (2, 1)):
        lat = synth.uniform(21, f"lat_{B}_{n}", (B, n, c["input_feat_dim"]), 1.0)
        exp = O.vocode_latents(w, c, lat)
        got = eng.forward_latents(lat.to(DEV), 4).cpu()
        assert got.shape == exp.shape
        np.testing.assert_allclose(got.numpy(), exp.numpy(), atol=1e-4)
    eng.close()


def test_hifigan_whole_call_graph_follows_the_callers_buffers(gold):
    """the whole call is one graph whose first and last kernel nodes carry the caller's pointers: different input / output
    tensors on every call (and both entry points) must be honoured"""
    from genvc_amd.engine import HifiganEngine
    g = gold("hifigan")
    seed = int(g["seed"])
    c = gcfg.DEFAULT_VOCODER
    eng = HifiganEngine(c, max_batch=2, max_frames=64)
    eng.bind(synth.make_weights(seed, synth.hifigan_weight_spec(c), device=DEV))
    ref = g["full_wav_1_8"]
    lat0 = synth.uniform(seed, "lat_1_8", (1, 8, c["input_feat_dim"]), 1.0).to(DEV)
    keep = []
    for i in range(4):
        lat = lat0.clone() if i % 2 else torch.cat([torch.zeros_like(lat0), lat0], 1)[:, 8:]      # fresh storage / an offset view
        wav = eng.forward_latents(lat.contiguous(), 4)
        keep.append(wav)
        other = eng.forward_latents((lat0 * 0.5).contiguous(), 4)                                # a different input in between
        assert float((other - wav).abs().max()) > 1e-3
    for wav in keep:
        np.testing.assert_allclose(wav.cpu().numpy(), ref, atol=1e-4)
    eng.close()


def test_hifigan_back_to_back_calls_without_sync_keep_their_own_buffers(gold):
    """streamed chunks are enqueued back to back with no host sync in between, each with other input / output
    pointers, so the executable graph of call N + 1 is prepared while call N may still be running.  A ring of executable graphs
    (a slot is only re-pointed once its previous launch has finished) keeps every call on its own buffers: 24 calls with 6
    different inputs and fresh outputs, enqueued in one go, each equal to the synchronous result"""
    from genvc_amd.engine import HifiganEngine
    g = gold("hifigan")
    seed = int(g["seed"])
    c = gcfg.DEFAULT_VOCODER
    eng = HifiganEngine(c, max_batch=2, max_frames=64)
    eng.bind(synth.make_weights(seed, synth.hifigan_weight_spec(c), device=DEV))
    lat0 = synth.uniform(seed, "lat_1_8", (1, 8, c["input_feat_dim"]), 1.0).to(DEV)
    lats = [(lat0 * (1.0 - 0.1 * i)).contiguous() for i in range(6)]
    sync = []
    for x in lats:
        sync.append(eng.forward_latents(x, 4).clone())
        torch.cuda.synchronize()
    np.testing.assert_allclose(sync[0].cpu().numpy(), g["full_wav_1_8"], atol=1e-4)
    outs = [eng.forward_latents(lats[i % 6], 4) for i in range(24)]            # no sync: 24 graph launches in flight / queued
    torch.cuda.synchronize()
    for i, w in enumerate(outs):
        assert torch.equal(w, sync[i % 6]), f"call {i} saw another call's buffers"
    eng.close()


def test_resampler_matches_oracle_restatement():
    """row f2: the polyphase sinc resampler kernel against the ORACLE's float64 restatement of torchaudio.functional.resample
    (oracle/genvc_oracle.py resample; torchaudio is absent from the image, so parity with torchaudio itself is unpinned)"""
    from oracle.genvc_oracle import resample as ref_resample
    from genvc_amd.engine import resample
    for orig, new, T in ((96000, 16000, 147486), (96000, 24000, 98835 * 4 // 4 + 3), (22050, 16000, 30000), (16000, 24000, 5000)):
        x = synth.synth_audio(9, f"rs{orig}", T)
        x = torch.cat([x, synth.synth_audio(10, f"rs{orig}", T, amplitude=0.3)], 0)
        got = resample(x.to(DEV), orig, new).cpu()
        ref = ref_resample(x, orig, new)
        assert got.shape == ref.shape
        np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=2e-5)


def test_hubert_matches_hf_golden_and_oracle(gold):
    """ContentVec forward (row f3): HIP path vs the HuggingFace HubertModel vectors and the oracle restatement"""
    from genvc_amd.engine import HubertEngine
    from oracle import genvc_oracle as O
    g = gold("hubert")
    seed = int(g["seed"])
    for tag, c in (("tiny", gcfg.TINY_HUBERT), ("full", gcfg.DEFAULT_HUBERT)):
        w = synth.make_weights(seed, synth.hubert_weight_spec(c), device=DEV)
        eng = HubertEngine(c, max_batch=2, max_samples=16000 * 7)
        eng.bind(w)
        for B, T in ((1, 16000), (2, 5120), (1, 24581)):
            wav = torch.cat([synth.synth_audio(seed + b, f"wav{T}", T) for b in range(B)], 0)
            got = eng.forward(wav.to(DEV)).cpu().numpy()
            ref = g[f"{tag}_feat_{B}_{T}"]
            assert got.shape[:2] == ref.shape[:2] and got.shape[-1] == 256
            np.testing.assert_allclose(got[:, :, :ref.shape[-1]], ref, atol=5e-4)      # fp32 tolerance, 12 post-LN layers
            # second call replays the captured graph
            np.testing.assert_array_equal(eng.forward(wav.to(DEV)).cpu().numpy(), got)
        # a length no golden vector covers, 6 s (the bench segment): against the oracle restatement
        wcpu = {k: v.cpu() for k, v in w.items()}
        wav = synth.synth_audio(seed + 5, "wav6s", 96000)
        got = eng.forward(wav.to(DEV)).cpu()
        ref = O.hubert_extract_features(wcpu, c, wav)
        assert got.shape == ref.shape == (1, 299, 256)
        np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=5e-4)
        eng.close()


def test_hubert_other_configuration_matches_oracle():
    """row f3 beyond HuBERT-base: 256-channel feature extractor (another instance of the one-round-trip conv kernel for the short
    layers), 256-wide encoder with 4 heads, batches of 1-3 at lengths either side of the conv kernel's frame limit"""
    from genvc_amd.engine import HubertEngine
    from oracle import genvc_oracle as O
    c = dict(conv_layers=[(256, 10, 5)] + [(256, 3, 2)] * 4 + [(256, 2, 2)] * 2, embed_dim=256, layers=3, heads=4, ffn_dim=512,
             pos_conv_kernel=128, pos_conv_groups=16, final_dim=256)
    w = synth.make_weights(41, synth.hubert_weight_spec(c))
    eng = HubertEngine(c, max_batch=3, max_samples=16000 * 5)
    eng.bind({k: v.to(DEV) for k, v in w.items()})
    for B, T in ((1, 16000), (3, 16000), (2, 70000), (1, 8000)):
        wav = torch.cat([synth.synth_audio(41 + b, f"wav{T}", T) for b in range(B)], 0)
        ref = O.hubert_extract_features(w, c, wav)
        got = eng.forward(wav.to(DEV)).cpu()
        assert got.shape == ref.shape
        np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=5e-4)
    eng.close()


def test_hubert_rejects_short_and_oversized_input():
    from genvc_amd.engine import HubertEngine
    from genvc_amd._lib import GenvcHipError
    c = gcfg.TINY_HUBERT
    eng = HubertEngine(c, max_batch=1, max_samples=16000)
    eng.bind(synth.make_weights(3, synth.hubert_weight_spec(c), device=DEV))
    assert eng.frames(16000) == 49 and eng.frames(400) == 1 and eng.frames(399) == 0
    with pytest.raises(ValueError):
        eng.forward(torch.zeros(1, 399, device=DEV))
    with pytest.raises(GenvcHipError):
        eng.forward(torch.zeros(1, 16001, device=DEV))
    with pytest.raises(GenvcHipError):
        eng.forward(torch.zeros(2, 8000, device=DEV))


def test_hubert_batches_agree_with_single_items():
    """batch invariance across the transformer paths: 2 x 49 frames (skinny, 7 M-tiles), 3 x 49 (tiled), 1 x 49 (skinny, 4)"""
    from genvc_amd.engine import HubertEngine
    c = gcfg.DEFAULT_HUBERT
    eng = HubertEngine(c, max_batch=3, max_samples=16000)
    eng.bind(synth.make_weights(17, synth.hubert_weight_spec(c), device=DEV))
    wav = torch.cat([synth.synth_audio(30 + b, "w", 16000) for b in range(3)], 0).to(DEV)
    solo = [eng.forward(wav[b:b + 1].contiguous()) for b in range(3)]
    for B in (2, 3):
        got = eng.forward(wav[:B].contiguous())
        for b in range(B):
            np.testing.assert_allclose(got[b].cpu().numpy(), solo[b][0].cpu().numpy(), atol=2e-5)
    eng.close()


def test_hubert_padding_mask_follows_zero_runs():
    """content_processor.py:24: padding_mask = (wav == 0).  Frames whose whole chunk of samples is exactly zero are padding
    (fairseq forward_padding_mask): their rows are zeroed ahead of the positional conv and their keys are excluded from
    every attention.  Cases: the harness's zero-padded tail segment (5120 samples, 2000 of them real), an interior run of
    digital silence, a batch whose items have different masks, and isolated zero samples (no frame is padding)."""
    from genvc_amd.engine import HubertEngine
    from oracle import genvc_oracle as O
    for c, T in ((gcfg.TINY_HUBERT, 16000), (gcfg.DEFAULT_HUBERT, 16000)):
        w = synth.make_weights(23, synth.hubert_weight_spec(c), device=DEV)
        wcpu = {k: v.cpu() for k, v in w.items()}
        eng = HubertEngine(c, max_batch=2, max_samples=T)
        eng.bind(w)
        tail = torch.zeros(1, 5120)
        tail[:, :2000] = synth.synth_audio(41, "tail", 2000)
        silence = synth.synth_audio(42, "mid", T).clone()
        silence[:, 5000:9000] = 0.0                                   # covers whole chunks of 326 samples -> padding frames
        sparse = synth.synth_audio(43, "sp", T).clone()
        sparse[:, ::7] = 0.0                                          # zeros, but no all-zero chunk
        for wav in (tail, silence, torch.cat([silence, sparse], 0), sparse):
            F_ = eng.frames(wav.shape[1])
            pm = O.hubert_frame_padding_mask(wav, F_)
            ref = O.hubert_extract_features(wcpu, c, wav)
            got = eng.forward(wav.to(DEV)).cpu()
            np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=5e-4)
            nomask = O.hubert_extract_features(wcpu, c, wav, padding_mask=False)
            if bool(pm.any()):                                        # the mask matters: the mask-free forward is far away
                assert float((nomask - ref).abs().max()) > 1e-2
            else:
                assert torch.equal(nomask, ref)
        assert int(O.hubert_frame_padding_mask(tail, eng.frames(5120)).sum()) >= 8
        assert int(O.hubert_frame_padding_mask(silence, 49).sum()) >= 10
        eng.close()
