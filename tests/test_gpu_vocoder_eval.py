"""GPU parity of the vocoder evaluation step: MultiScaleDiscriminator / MultiPeriodDiscriminator, the criteria and the mel loss against
the reference's own classes (tests/golden/vocoder_eval.npz, scripts/make_vocoder_eval_golden.py) and their CPU restatement
(tests/vocoder_eval_oracle.py).

Tolerance: 8 x floor per quantity.  A floor is max(max|fp32 - fp64| of the reference (fixture) or of the oracle (edge shapes),
2^-24 max|value|): what fp32 arithmetic in another summation order costs, and never less than half an ulp of the largest entry.  One
measured maximum is not a bound, hence the factor 8."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vocoder_eval_oracle as VO      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 8.0


def build_msd(max_batch=3, max_samples=4096):
    from genvc_amd.layers.hifigan import MultiScaleDiscriminator
    m = MultiScaleDiscriminator()
    m.load_state_dict(VO.msd_weights(device=DEV), strict=True)
    return m.to(DEV).eval().bind(max_batch=max_batch, max_samples=max_samples)


def build_mpd(cfg, max_batch=3, max_samples=4096):
    from genvc_amd.layers.hifigan import MultiPeriodDiscriminator
    m = MultiPeriodDiscriminator(cfg["mpd_reshapes"], cfg["mpd_discriminator_channel_mult_factor"], cfg["mpd_use_spectral_norm"])
    m.load_state_dict(VO.mpd_weights(cfg, device=DEV), strict=True)
    return m.to(DEV).eval().bind(max_batch=max_batch, max_samples=max_samples)


@pytest.fixture(scope="module")
def msd():
    m = build_msd()
    yield m
    m._engine.close()


@pytest.fixture(scope="module")
def mpd_small():
    m = build_mpd(VO.mpd_cfg(0.25))
    yield m
    m._engine.close()


def quantities(outs, sub=False):
    """every compared quantity of one discriminator call -> {name: float64 ndarray} (the fixture's names)"""
    from genvc_amd.layers import hifigan_loss as HL
    d_r, d_g, f_r, f_g = outs
    device = isinstance(d_r[0], torch.Tensor) and d_r[0].is_cuda
    n = lambda t: t.detach().double().cpu().numpy()                      # noqa: E731
    keep = VO.subsample if sub else (lambda t: t)
    q = {}
    for i in range(len(d_r)):
        q[f"dr{i}"], q[f"dg{i}"] = n(d_r[i]), n(d_g[i])
        for l in range(len(f_r[i])):
            q[f"fr{i}_{l}"], q[f"fg{i}_{l}"] = n(keep(f_r[i][l])), n(keep(f_g[i][l]))
    if device:
        q["fmean"] = n(d_r.stats[:, 3:])
        loss, rl, gl = HL.discriminator_criterion()(d_r, d_g)
        gen, genl = HL.generator_criterion()(d_g)
        feat = HL.feature_criterion()(f_r, f_g)
        assert loss.is_cuda and gen.is_cuda and feat.is_cuda
    else:
        q["fmean"] = np.array([[float(v) for v in row] for row in VO.feature_means(f_r, f_g)], dtype=np.float64)
        loss, rl, gl = VO.discriminator_criterion(d_r, d_g)
        gen, genl = VO.generator_criterion(d_g)
        feat = VO.feature_criterion(f_r, f_g)
    q["disc"], q["rl"], q["gl"] = n(loss), np.array(rl, dtype=np.float64), np.array(gl, dtype=np.float64)
    q["gen"], q["genl"], q["feat"] = n(gen), np.array([float(v) for v in genl], dtype=np.float64), n(feat)
    return q


def compare(label, got, want, floor_of):
    worst, worst_k = 0.0, None
    for k, w in want.items():
        assert got[k].shape == w.shape, (label, k, got[k].shape, w.shape)
        fl = np.asarray(floor_of(k), dtype=np.float64)                 # a scalar, or one floor per entry (fmean)
        ratio = float((np.abs(got[k] - w) / fl).max())
        if ratio > worst:
            worst, worst_k = ratio, k
        assert ratio <= MARGIN, f"{label} {k}: |device - reference| is {ratio:.2f} floors (floor {fl.max():.3e}), more than {MARGIN:g}"
    print(f"{label}: {len(want)} quantities, worst {worst:.2f} floors ({worst_k})")


@pytest.mark.parametrize("tag,B,T,mult", VO.CASES)
def test_discriminators_match_reference(gold, msd, mpd_small, tag, B, T, mult):
    g = gold("vocoder_eval")
    y, y_hat = VO.wav_pair(int(g["seed"]), B, T, DEV)
    mpd = build_mpd(VO.mpd_cfg(mult)) if mult != 0.25 else mpd_small
    try:
        for D, model in (("msd", msd), ("mpd", mpd)):
            assert list(model.state_dict().keys()) == [str(k) for k in g[f"{tag}_{D}_keys"]]
            got = quantities(model(y, y_hat), sub=True)
            pre = f"{tag}_{D}_"
            want = {k[len(pre):]: g[k].astype(np.float64) for k in g.files if k.startswith(pre) and k[len(pre)] != "w" and not k.endswith("keys")}
            assert len(want) == len(got)
            compare(f"{tag} {D} B={B} T={T}", got, want, lambda k: g[f"floor_{pre}{k}"])
            # the folds: the engine's folded weights against the reference's
            for k in g.files:
                if k.startswith(pre + "w"):
                    i, l = (int(v) for v in k[len(pre) + 1:].split("_"))
                    conv = model.discriminators[i].conv_post if l == len(model.discriminators[i].convs) else model.discriminators[i].convs[l]
                    shape = (conv.weight_orig if hasattr(conv, "weight_orig") else conv.weight_v).shape
                    w = model._engine.folded_weight(i, l, shape).reshape(-1)[:64].cpu().numpy()
                    np.testing.assert_allclose(w, g[k], rtol=2e-6, atol=0)       # (a 2624-term fp32 norm / sigma in another order)
    finally:
        if mpd is not mpd_small:
            mpd._engine.close()


def oracle_reference(fn, w, y, y_hat):
    """oracle in fp32 and the floors from its fp64 run"""
    q32 = quantities(fn(w, y.cpu(), y_hat.cpu()))
    w64 = {k: v.double() for k, v in w.items()}
    q64 = quantities(fn(w64, y.cpu().double(), y_hat.cpu().double()))
    floors = {k: max(float(np.abs(q32[k] - q64[k]).max()), 2.0 ** -24 * float(np.abs(q64[k]).max())) for k in q32}
    # fmean entry by entry, as in the fixture: a mean over a map moves by at most the sum of its two maps' floors
    n_sub, n_layers = q32["fmean"].shape
    maps = np.array([[floors[f"fr{i}_{l}"] + floors[f"fg{i}_{l}"] for l in range(n_layers)] for i in range(n_sub)])
    floors["fmean"] = np.maximum(maps, np.maximum(np.abs(q32["fmean"] - q64["fmean"]), 2.0 ** -24 * np.abs(q64["fmean"])))
    return q32, floors


@pytest.fixture(scope="module")
def msd_w():
    return VO.msd_weights()


# T = 1024: one code; 1031: prime, every period pads; 100: the last MSD scale is down to 1 frame from its fifth conv on; B = 3
@pytest.mark.parametrize("B,T", [(1, 1024), (2, 1031), (1, 100), (3, 1500)])
def test_edge_shapes_match_oracle(msd, mpd_small, msd_w, B, T):
    y, y_hat = VO.wav_pair(5, B, T, DEV)
    with torch.inference_mode():
        want, floors = oracle_reference(lambda w, a, b: VO.msd(w, a, b), msd_w, y, y_hat)
        compare(f"msd B={B} T={T}", quantities(msd(y, y_hat)), want, floors.__getitem__)
        cfg = VO.mpd_cfg(0.25)
        want, floors = oracle_reference(lambda w, a, b: VO.mpd(w, cfg["mpd_reshapes"], a, b), VO.mpd_weights(cfg), y, y_hat)
        compare(f"mpd B={B} T={T}", quantities(mpd_small(y, y_hat)), want, floors.__getitem__)


@pytest.mark.parametrize("cfg", [VO.mpd_cfg(0.25, periods=(2, 3)), VO.mpd_cfg(0.25, spectral=True)], ids=["periods_2_3", "spectral_norm"])
def test_mpd_variants_match_oracle(cfg):
    m = build_mpd(cfg, max_batch=2, max_samples=2048)
    try:
        y, y_hat = VO.wav_pair(6, 2, 2000, DEV)
        with torch.inference_mode():
            want, floors = oracle_reference(lambda w, a, b: VO.mpd(w, cfg["mpd_reshapes"], a, b), VO.mpd_weights(cfg), y, y_hat)
        compare(f"mpd {cfg}", quantities(m(y, y_hat)), want, floors.__getitem__)
    finally:
        m._engine.close()


def test_training_mode_and_unserved_discriminators_raise(mpd_small):
    from genvc_amd.layers import hifigan as H
    y, y_hat = VO.wav_pair(5, 1, 1024, DEV)
    mpd_small.train()
    try:
        with pytest.raises(NotImplementedError):
            mpd_small(y, y_hat)
    finally:
        mpd_small.eval()
    for cls in (H.MultiScaleSTFTDiscriminator, H.MultiScaleSubbandCQTDiscriminator):
        with pytest.raises(NotImplementedError, match=cls.__name__):
            cls()


# ---- mel loss ----------------------------------------------------------------------------------------------------------------------
def test_mel_loss_matches_reference(gold):
    from genvc_amd.layers.hifigan_loss import mel_criterion
    g = gold("vocoder_eval")
    y, y_hat = VO.wav_pair(int(g["seed"]), 2, 4096, DEV)
    crit = mel_criterion(VO.MEL_CFG)
    feat = crit.extract_mel_features(y)
    assert feat.shape == (2, 100, 16)
    e_feat = float(np.abs(feat[0].double().cpu().numpy() - g["mel_feat"]).max())
    loss = crit(y, y_hat)
    e_loss = abs(float(loss) - float(g["mel_loss"]))
    print(f"mel: max |features - reference| {e_feat:.3e} (floor {float(g['floor_mel_feat']):.3e}), loss {float(loss):.6f} vs "
          f"{float(g['mel_loss']):.6f}: {e_loss:.3e} (floor {float(g['floor_mel_loss']):.3e})")
    assert e_feat <= MARGIN * float(g["floor_mel_feat"])
    assert e_loss <= MARGIN * float(g["floor_mel_loss"])


@pytest.mark.parametrize("B,T", [(1, 4096), (2, 1000), (3, 385)])
def test_mel_loss_matches_oracle(B, T):
    """B = 1 is the natural definition (the reference's y.squeeze() drops the batch axis there and its own padding call fails)"""
    from genvc_amd.layers.hifigan_loss import mel_criterion
    y, y_hat = VO.wav_pair(8, B, T, DEV)
    crit = mel_criterion(VO.MEL_CFG)
    feat, loss = crit.extract_mel_features(y).double().cpu(), float(crit(y, y_hat))
    o32, o64 = VO.extract_mel_features(y.cpu().reshape(B, T)), VO.extract_mel_features(y.cpu().reshape(B, T).double())
    l32, l64 = float(VO.mel_criterion(y.cpu(), y_hat.cpu())), float(VO.mel_criterion(y.cpu().double(), y_hat.cpu().double()))
    f_floor = max(float((o32.double() - o64).abs().max()), 2.0 ** -24 * float(o64.abs().max()))
    l_floor = max(abs(l32 - l64), 2.0 ** -24 * abs(l64))
    e_feat, e_loss = float((feat - o32.double()).abs().max()), abs(loss - l32)
    print(f"mel B={B} T={T}: features {e_feat:.3e} (floor {f_floor:.3e}), loss {e_loss:.3e} (floor {l_floor:.3e})")
    assert feat.shape == o32.shape == (B, 100, T // 256)
    assert e_feat <= MARGIN * f_floor and e_loss <= MARGIN * l_floor


def test_mel_loss_rejects_short_input():
    from genvc_amd.layers.hifigan_loss import mel_criterion
    y, y_hat = VO.wav_pair(8, 1, 384, DEV)
    with pytest.raises(ValueError):
        mel_criterion(VO.MEL_CFG)(y, y_hat)


# ---- determinism -------------------------------------------------------------------------------------------------------------------
def test_losses_are_bit_stable_and_calls_keep_their_results(msd, mpd_small):
    from genvc_amd.layers.hifigan_loss import mel_criterion
    a, a_hat = VO.wav_pair(9, 2, 1500, DEV)
    b, b_hat = VO.wav_pair(10, 1, 1031, DEV)
    crit = mel_criterion(VO.MEL_CFG)
    for model in (msd, mpd_small):
        s1 = model(a, a_hat)[0].stats
        s2 = model(b, b_hat)[0].stats                 # a second shape right behind the first, no sync in between
        s3 = model(a, a_hat)[0].stats                 # and the first again: re-planned correctly, bit-identical
        torch.cuda.synchronize()
        assert torch.equal(s1, s3) and s1.shape == s2.shape and not torch.equal(s1, s2)
        s4 = model(b, b_hat)[0].stats
        assert torch.equal(s2, s4)
    m1, m2, m3 = crit(a, a_hat), crit(b, b_hat), crit(a, a_hat)
    torch.cuda.synchronize()
    assert torch.equal(m1, m3) and not torch.equal(m1, m2)


# ---- evaluate_vocoder --------------------------------------------------------------------------------------------------------------
def test_evaluate_vocoder_composes():
    """the wav -> generated-waveform part is pinned stage by stage elsewhere; here the device's own generated waveform and padded wav
    go through the oracle's discriminators and criteria and must give the device's loss_disc and mel_loss"""
    from genvc_amd import config as gcfg
    from genvc_amd import synth
    from genvc_amd.inference.model_init import model_init_synthetic
    cfg = gcfg.default_config(tiny=True, with_acoustic=True)
    model, _ = model_init_synthetic(cfg, seed=3, device=DEV, max_slots=2)
    # (the reference's step needs ceil((T + 512) / 1024) latents = the audio-code count: T mod 1024 in [0, 512])
    B, T = 2, 11520
    lens = [T, T - 2000]
    wav = torch.zeros(B, 1, T)
    for b, n in enumerate(lens):
        wav[b, 0, :n] = synth.synth_audio(40 + b, "ev_wav", n, amplitude=0.3)[0]
    wav = wav.to(DEV)
    cond = torch.stack([synth.synth_audio(50 + b, "ev_cond", 12000) for b in range(B)]).unsqueeze(1).to(DEV)      # [2,1,1,12000]
    wav_lengths = torch.tensor(lens, device=DEV)

    def batch():
        return dict(wav=wav.clone(), wav_lengths=wav_lengths.clone(), conditioning=cond.clone(), cond_lens=torch.tensor([12000, 12000]))

    # synthetic discriminator weights (the engines are bound at the first forward)
    model._vocoder_discriminator("MSD").load_state_dict(VO.msd_weights(device=DEV), strict=True)
    model._vocoder_discriminator("MPD").load_state_dict(VO.mpd_weights(VO.mpd_cfg(0.25), device=DEV), strict=True)
    fb = model.format_vocoder_batch_on_device(batch())
    stride = cfg.model_args.gpt_code_stride_len
    n_codes = fb["mel_latents"].shape[1]
    assert n_codes == 12 and fb["wav"].shape == (B, 1, n_codes * stride)
    assert torch.equal(fb["wav"][:, :, :min(T, n_codes * stride)], wav[:, :, :min(T, n_codes * stride)]) and float(fb["wav"][:, :, T:].abs().sum()) == 0.0
    assert torch.equal(fb["wav_lengths"], wav_lengths + stride // 2)
    for k in ("cond_mels", "cond_lens", "audio_codes", "text_lengths", "text_inputs", "conditioning"):
        assert k not in fb
    res = model.evaluate_vocoder(batch(), return_audio=True)
    assert res["discriminators"] == ("MSD", "MPD")
    audio_gt, audio_pred = res["audio_gt"].cpu(), res["audio_pred"].cpu()
    assert audio_pred.shape == audio_gt.shape == fb["wav"].shape
    with torch.inference_mode():
        d_r, d_g, _, _ = VO.msd(VO.cpu_state(model.hifigan_discriminator["MSD"]), audio_gt, audio_pred)
        msd_loss = float(VO.discriminator_criterion(d_r, d_g)[0])
        mcfg = model.hifigan_discriminator["MPD"]
        d_r, d_g, _, _ = VO.mpd(VO.cpu_state(mcfg), mcfg.mpd_reshapes, audio_gt, audio_pred)
        mpd_loss = float(VO.discriminator_criterion(d_r, d_g)[0])
        mel = float(VO.mel_criterion(audio_gt, audio_pred))
    print(f"evaluate_vocoder: MSD {res['MSD_Discriminator_loss']:.6f} vs {msd_loss:.6f}, MPD {res['MPD_Discriminator_loss']:.6f} vs "
          f"{mpd_loss:.6f}, mel {res['mel_loss']:.6f} vs {mel:.6f}")
    # sums of 3 / 5 means of squares of O(1) logits and 45 x an O(1) mean: 2e-4, the bar of the other evaluation passes' losses
    assert abs(res["MSD_Discriminator_loss"] - msd_loss) <= 2e-4 and abs(res["MPD_Discriminator_loss"] - mpd_loss) <= 2e-4
    assert abs(res["loss_disc"] - (msd_loss + mpd_loss)) <= 4e-4 and abs(res["mel_loss"] - mel) <= 2e-4 * max(1.0, abs(mel))
    with pytest.raises(NotImplementedError, match="MSTFT"):
        model.evaluate_vocoder(batch(), discriminators=("MSD", "MSTFT"))
    with pytest.raises(NotImplementedError, match="MSCQT"):
        model.evaluate_vocoder(batch(), discriminators=("MSCQT",))
