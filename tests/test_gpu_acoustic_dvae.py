"""GPU parity of the acoustic DiscreteVAE (decode, tokeniser, eval-mode forward) against the reference's own class
(tests/golden/acoustic_dvae_*.npz, scripts/make_acoustic_dvae_golden.py) and its CPU restatement (tests/dvae_full_oracle.py).

Bars: 1e-4 absolute on mels / decoder outputs (magnitude <= ~2.6), the project's mel bar; 2e-4 on the two losses (the bar of the
GPT.forward evaluation pass)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_full_oracle as DO      # noqa: E402
from genvc_amd import synth        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL = 1e-4
LOSS_ATOL = 2e-4
CFG = {"tiny": DO.TINY, "full": DO.FULL}
PRE_STEP = {"tiny": 1, "full": 8}
DECODE_ORDER = {"tiny": [(1, 71), (1, 1), (3, 33), (1, 2), (2, 5)], "full": [(2, 71), (1, 24)]}      # the geometry changes between calls
TOK_SAMPLES = [6000, 24077, 72000]


def build_dvae(cfg, seed, max_batch=3, max_frames=288):
    from genvc_amd.layers.dvae import DiscreteVAE
    m = DiscreteVAE(channels=cfg["num_channels"], normalization=None, positional_dims=1, num_tokens=cfg["num_tokens"],
                    codebook_dim=cfg["codebook_dim"], hidden_dim=cfg["hidden_dim"], num_resnet_blocks=cfg["num_resnet_blocks"],
                    kernel_size=cfg["kernel_size"], num_layers=cfg["num_layers"], use_transposed_convs=False, with_decoder=True)
    w = synth.make_weights(seed, synth.dvae_full_weight_spec(cfg, codebook_scale=DO.CODEBOOK_SCALE), device=DEV)
    m.load_state_dict(w, strict=True)
    m.to(DEV).eval()
    return m.bind(max_batch=max_batch, max_frames=max_frames)


@pytest.fixture(scope="module", params=["tiny", "full"])
def case(request, gold):
    tag = request.param
    g = gold(f"acoustic_dvae_{tag}")
    m = build_dvae(CFG[tag], int(g["seed"]), max_batch=8)
    yield tag, g, m
    m._engine.close()


def test_decode_matches_reference(case):
    tag, g, m = case
    seed, worst = int(g["seed"]), 0.0
    for B, n in DECODE_ORDER[tag]:
        codes = DO.designed_codes(seed, B, n, CFG[tag]["num_tokens"])
        out, pre = m.decode(codes.to(DEV))
        assert out.shape == (B, 80, 4 * n) and pre.shape == (B, CFG[tag]["hidden_dim"], 4 * n)
        e_out = np.abs(out.cpu().numpy() - g[f"dec_out_{B}_{n}"]).max()
        e_pre = np.abs(pre.cpu().numpy()[:, ::PRE_STEP[tag]] - g[f"dec_pre_{B}_{n}"]).max()
        print(f"decode {tag} {B}x{n}: max |out - ref| {e_out:.2e}, max |pre - ref| {e_pre:.2e}")
        worst = max(worst, e_out, e_pre)
        assert e_out <= ATOL and e_pre <= ATOL, (tag, B, n, e_out, e_pre)
    print(f"decode {tag}: worst {worst:.2e}")


def test_decode_kernel5_three_layers():
    seed = 13
    m = build_dvae(DO.K5, seed, max_batch=2, max_frames=96)
    codes = DO.designed_codes(seed, 2, 12, DO.K5["num_tokens"])
    out, pre = m.decode(codes.to(DEV))
    w = {k: v.cpu() for k, v in m.state_dict().items()}
    r_out, r_pre = DO.decode(w, DO.K5, codes)
    assert out.shape == r_out.shape == (2, 80, 96)
    e_out, e_pre = float((out.cpu() - r_out).abs().max()), float((pre.cpu() - r_pre).abs().max())
    print(f"decode k5: {e_out:.2e} {e_pre:.2e}")
    assert e_out <= ATOL and e_pre <= ATOL
    m._engine.close()


def test_decode_both_gemm_regimes(case):
    """The decoder has one conv path, the tiled GEMM, which splits K below 128 output tiles (launch_gemm_cap): one 71-code item per
    call stays below that at every layer, eight per call are above it.  Both agree with the reference and with each other."""
    tag, g, m = case
    seed = int(g["seed"])
    codes = DO.designed_codes(seed, 2, 71, CFG[tag]["num_tokens"]) if tag == "full" else DO.designed_codes(seed, 1, 71, CFG[tag]["num_tokens"])
    ref = g["dec_out_2_71"] if tag == "full" else g["dec_out_1_71"]
    big = codes.repeat(8 // codes.shape[0], 1).to(DEV)
    out8, _ = m.decode(big)
    for b in (0, 7):
        r = b % codes.shape[0]
        out1, _ = m.decode(big[b:b + 1].contiguous())
        assert np.abs(out1.cpu().numpy()[0] - ref[r]).max() <= ATOL
        assert np.abs(out8[b].cpu().numpy() - ref[r]).max() <= ATOL
        assert float((out1[0] - out8[b]).abs().max()) <= ATOL


def test_tokeniser_end_to_end(case, gold):
    from genvc_amd.utils import TorchMelSpectrogram
    tag, g, m = case
    seed = int(g["seed"])
    mel_gold = gold("acoustic_dvae_tiny") if tag == "tiny" else None
    mel_fn = TorchMelSpectrogram(filter_length=1024, hop_length=256, win_length=1024, sampling_rate=24000, mel_fmin=0, mel_fmax=8000,
                                 n_mel_channels=80)
    norms = mel_fn.mel_norms
    n_all = n_safe = n_exempt_diff = 0
    for n in TOK_SAMPLES:
        wav = DO.acoustic_wavs(seed, "wav", n)
        mel = mel_fn(wav.to(DEV))
        ref_mel = mel_gold[f"mel_{n}"] if mel_gold is not None else DO.mel_1024(wav, norms).numpy()
        e_mel = np.abs(mel.cpu().numpy() - ref_mel).max()
        print(f"tokeniser {tag} {n}: max |mel - ref| {e_mel:.2e}")
        assert e_mel <= ATOL
        codes = m.get_codebook_indices(mel).cpu().numpy()
        ref = g[f"tok_codes_{n}"]
        assert codes.shape == ref.shape
        safe = g[f"tok_margin_{n}"] > 1e-4
        n_all += safe.size; n_safe += int(safe.sum())
        assert np.array_equal(codes[safe], ref[safe])
        n_exempt_diff += int((codes[~safe] != ref[~safe]).sum())
    assert n_safe >= 0.97 * n_all
    print(f"tokeniser {tag}: {n_all} frames, {n_all - n_safe} with a reference margin <= 1e-4, {n_exempt_diff} of those differ")
    assert n_exempt_diff <= max(2, (n_all - n_safe) // 4)


def test_forward_matches_reference_and_is_deterministic(case):
    from genvc_amd.utils import DEFAULT_MEL_NORM_FILE, load_mel_norms
    tag, g, m = case
    seed = int(g["seed"])
    ref_out = g["fwd_out"]
    B, _, T = ref_out.shape
    norms = torch.from_numpy(load_mel_norms(DEFAULT_MEL_NORM_FILE))
    feat = DO.mel_1024(DO.acoustic_wavs(seed, "fwd", (T - 1) * 256 + 80, B), norms).to(DEV)
    recon, commit, out = m(feat)
    assert recon.dim() == 0 and commit.dim() == 0 and out.shape == ref_out.shape
    e_out = np.abs(out.cpu().numpy() - ref_out).max()
    e_r, e_c = abs(float(recon) - float(g["fwd_recon"])), abs(float(commit) - float(g["fwd_commit"]))
    print(f"forward {tag}: max |out - ref| {e_out:.2e}, recon {float(recon):.6f} (ref {float(g['fwd_recon']):.6f}), "
          f"commitment {float(commit):.6f} (ref {float(g['fwd_commit']):.6f})")
    assert np.array_equal(m.get_codebook_indices(feat).cpu().numpy(), g["fwd_codes"])       # (every frame's margin > 1e-4)
    assert e_out <= ATOL
    assert e_r <= LOSS_ATOL and e_c <= LOSS_ATOL
    recon2, commit2, out2 = m(feat)
    assert torch.equal(recon, recon2) and torch.equal(commit, commit2) and torch.equal(out, out2)
    i_out, i_pre = m.infer(feat)
    d_out, d_pre = m.decode(m.get_codebook_indices(feat))
    assert torch.equal(i_out, d_out) and torch.equal(i_pre, d_pre)
    assert torch.equal(i_out, out)
    with pytest.raises(ValueError):
        m(feat[:, :, :T - 2].contiguous())


def test_out_of_range_codes_raise(case):
    tag, g, m = case
    seed = int(g["seed"])
    B, n = (2, 5) if tag == "tiny" else (1, 24)
    codes = DO.designed_codes(seed, B, n, CFG[tag]["num_tokens"]).to(DEV)
    for bad in (CFG[tag]["num_tokens"], -1):
        c = codes.clone()
        c[-1, n // 2] = bad
        with pytest.raises(ValueError):
            m.decode(c)
        out, _ = m.decode(codes)
        assert np.abs(out.cpu().numpy() - g[f"dec_out_{B}_{n}"]).max() <= ATOL


def test_model_evaluate_from_waveforms():
    """GenVCModel.evaluate on a tiny synthetic model: B = 2, wavs of 1.0 s and 0.6 s, one 0.5 s conditioning clip each"""
    from genvc_amd import config as gcfg
    from genvc_amd.inference.inference_utils import synthesize_utt
    from genvc_amd.inference.model_init import model_init_synthetic
    from genvc_amd.layers.dvae import DiscreteVAE
    from genvc_amd.utils import TorchMelSpectrogram
    m, _ = model_init_synthetic(gcfg.default_config(tiny=True, with_acoustic=True), seed=3, device=DEV, max_slots=2)
    assert m.acoustic_dvae._engine is None                       # bound on first use
    lens = [24000, 14400]
    wav = torch.zeros(2, 1, lens[0])
    for i, n in enumerate(lens):
        wav[i, 0, :n] = synth.synth_audio(40 + i, "eval_wav", n, amplitude=DO.WAV_AMPLITUDES[i])[0]
    cond = torch.stack([synth.synth_audio(50 + i, "eval_cond", 12000) for i in range(2)]).unsqueeze(1)      # [2,1,1,12000]

    def batch():
        return dict(wav=wav.clone().to(DEV), wav_lengths=torch.tensor(lens), conditioning=cond.clone().to(DEV),
                    cond_lens=torch.tensor([12000, 12000]))
    res = m.evaluate(batch())
    b = m.format_batch_on_device(batch())
    assert b["cond_mels"].shape == (2, 1, 80, 47) and b["audio_codes"].shape == (2, 24)
    assert b["text_lengths"].tolist() == [12, 7] and b["text_lengths"].dtype == torch.long
    # 1.0 s at 16 kHz + 320 zero samples -> 50 ContentVec frames -> 13 content codes
    assert b["text_inputs"].shape == (2, 13)
    lt, lm, acc, _ = m.gpt(b["text_inputs"], b["text_lengths"], b["audio_codes"], b["wav_lengths"], cond_mels=b["cond_mels"],
                           cond_lens=b["cond_lens"])
    assert torch.equal(res["loss_text_ce"], lt) and torch.equal(res["loss_mel_ce"], lm) and torch.equal(res["top10acc"], acc)
    assert torch.equal(res["loss"], 0.01 * lt + 1.0 * lm)
    assert all(bool(torch.isfinite(v)) for v in res.values()) and 0.0 <= float(acc) <= 1.0
    # the same wavs through a tokeniser of its own (the extractor and a DiscreteVAE with the model's tensors)
    ac = m.config.acoustic_dvae_config
    own = DiscreteVAE(channels=ac.num_channels, num_tokens=ac.num_tokens, codebook_dim=ac.codebook_dim, hidden_dim=ac.hidden_dim,
                      num_resnet_blocks=ac.num_resnet_blocks, kernel_size=ac.kernel_size, num_layers=ac.num_layers, positional_dims=1,
                      use_transposed_convs=False, with_decoder=True)
    own.load_state_dict(m.acoustic_dvae.state_dict(), strict=True)
    own.to(DEV).eval()
    mel = TorchMelSpectrogram(filter_length=1024, hop_length=256, win_length=1024, sampling_rate=24000, mel_fmin=0, mel_fmax=8000,
                              n_mel_channels=80)(wav.to(DEV))
    assert torch.equal(own.get_codebook_indices(mel), b["audio_codes"])
    assert int(b["audio_codes"].unique().numel()) >= 4
    # generated codes back to a mel
    out, _ = m.acoustic_dvae.decode(b["audio_codes"])
    assert out.shape == (2, 80, 96) and bool(torch.isfinite(out).all())
    own._engine.close()
    # a model without an acoustic config: as before, and no acoustic engine on it
    plain, _ = model_init_synthetic(gcfg.default_config(tiny=True), seed=3, device=DEV, max_slots=2)
    plain.config.top_k = 1
    plain.gpt.max_gen_mel_tokens = 16
    assert plain.acoustic_dvae is None and not hasattr(plain, "torch_mel_spectrogram_dvae")
    d = synthesize_utt(plain, synth.synth_audio(5, "src", 16000), synth.synth_audio(6, "ref", 48000), seg_len=1.0, return_details=True)
    assert bool(torch.isfinite(d["wav"]).all()) and d["wav"].numel() > 0
    with pytest.raises(NotImplementedError):
        plain.format_batch_on_device(batch())


def test_cli_decode_codes_to_mel(tmp_path):
    """infer.py --decode_codes_to_mel on the tiny synthetic model: one mel of 4 frames per generated code"""
    import subprocess
    from genvc_amd.audio import save_wav
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    save_wav(str(tmp_path / "src.wav"), synth.synth_audio(5, "src", 16000)[0], 16000)
    save_wav(str(tmp_path / "ref.wav"), synth.synth_audio(6, "ref", 48000)[0], 24000)
    r = subprocess.run([sys.executable, os.path.join(root, "infer.py"), "--synthetic", "--tiny", "--src_wav", str(tmp_path / "src.wav"),
                        "--ref_audio", str(tmp_path / "ref.wav"), "--output_path", str(tmp_path / "out.wav"), "--top_k", "1",
                        "--seg_len", "1.0", "--save_tokens", str(tmp_path / "tok.pt"), "--decode_codes_to_mel", str(tmp_path / "mel.npy")],
                       capture_output=True, text=True, cwd=root, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    mel = np.load(str(tmp_path / "mel.npy"))
    tok = torch.load(str(tmp_path / "tok.pt"))["tokens"]
    n = int((tok < 1024).sum())
    assert mel.shape == (80, 4 * n) and n > 0 and np.isfinite(mel).all()
