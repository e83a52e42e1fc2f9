"""GPU parity of TorchMelSpectrogram.invert -- the inverse mel scale and Griffin-Lim of csrc/griffinlim.hip -- against their CPU
restatement (tests/griffinlim_oracle.py).

Tolerance: |device - oracle fp32| <= 8 x floor, floor = max(max|oracle fp32 - oracle fp64|, 2^-24 max|value|): what fp32 arithmetic in
another order costs, and never less than half an ulp of the largest entry.  One measured maximum is not a bound, hence the factor 8.
For 64 iterations the fp32-against-fp64 difference of ONE run does not bound 64 phase projections, so the floor is the largest of that
difference, the fp64 oracle's own spread over 4 runs whose start phases are each rotated by +-2^-22 rad (two ulps of a unit phasor's
components: the size of a rounding of the start), and 2^-24 max|wav|.  Every floor is computed here from the CPU oracle and printed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import griffinlim_oracle as GO      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 8.0


def check(label, got, w32, w64, extra_floor=0.0):
    """|got - w32| against 8 floors; prints the figures before it asserts"""
    got = got.detach().double().cpu()
    assert got.shape == w32.shape, (label, got.shape, w32.shape)
    floor = max(GO.floor_of(w32, w64), extra_floor)
    err = float((got - w32.double()).abs().max())
    print(f"{label}: max|device - oracle32| {err:.3e}, floor {floor:.3e} ({err / floor:.2f} floors), max|value| {float(w64.abs().max()):.3e}")
    assert bool(torch.isfinite(got).all()), label
    assert err <= MARGIN * floor, f"{label}: {err:.3e} is {err / floor:.2f} floors (floor {floor:.3e}), more than {MARGIN:g}"
    return err, floor


@pytest.fixture(scope="module")
def engines():
    """one engine per STFT geometry; 20 mels at n_fft 512, whose 257 bins cannot carry 80 filters"""
    from genvc_amd.engine import GriffinLimEngine
    made = {}

    def get(n_fft, win, hop):
        key = (n_fft, win, hop)
        if key not in made:
            made[key] = GriffinLimEngine(None, n_fft=n_fft, hop=hop, win=win, sample_rate=24000, f_min=0.0, f_max=8000.0,
                                         n_mels=80 if n_fft >= 1024 else 20, max_batch=2, max_frames=16)
        return made[key]
    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def norms():
    from genvc_amd.utils import DEFAULT_MEL_NORM_FILE, load_mel_norms
    return torch.from_numpy(load_mel_norms(DEFAULT_MEL_NORM_FILE))


@pytest.mark.parametrize("cfg", GO.DVAE_MELS, ids=["24000", "22050"])
def test_inverse_matrix_is_the_pseudo_inverse(cfg):
    """W is built in double and stored as fp32: every entry within half an fp32 ulp of the fp64 pseudo-inverse's (the double Cholesky's own
    error, condition number 5.4 squared times 2^-53, is allowed for by 1e-10 of the largest entry)"""
    from genvc_amd.engine import GriffinLimEngine
    eng = GriffinLimEngine(None, max_batch=1, max_frames=2, **cfg)
    try:
        W = eng.inverse_matrix()
    finally:
        eng.close()
    fb = GO.filterbank(cfg["n_fft"], cfg["sample_rate"], cfg["f_min"], cfg["f_max"], cfg["n_mels"], torch.float64)
    pinv = torch.linalg.pinv(fb.T)
    assert W.shape == pinv.shape == (cfg["n_fft"] // 2 + 1, cfg["n_mels"]) and W.dtype == torch.float32
    bound = 2.0 ** -24 * pinv.abs() + 1e-10 * float(pinv.abs().max())
    err = (W.double() - pinv).abs()
    print(f"inverse matrix {cfg['sample_rate']}: max|W - pinv| {float(err.max()):.3e}, max|pinv| {float(pinv.abs().max()):.3e}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("with_norms", [True, False], ids=["norms", "no_norms"])
@pytest.mark.parametrize("cfg", GO.DVAE_MELS, ids=["24000", "22050"])
def test_inverse_mel_matches_oracle(cfg, with_norms, norms):
    from genvc_amd.engine import GriffinLimEngine
    B, F = 2, 3
    g = torch.Generator().manual_seed(21)
    logp = torch.rand(B, cfg["n_mels"], F, generator=g) * 13.5 - 11.5               # log power between the clamp 1e-5 and e^2
    nrm = norms if with_norms else None
    mel = logp / norms.view(1, -1, 1) if with_norms else logp
    eng = GriffinLimEngine(None if nrm is None else nrm.numpy(), max_batch=1, max_frames=2, **cfg)
    try:
        got = eng.inverse_mel(mel.to(DEV))
    finally:
        eng.close()
    w32, w64 = (GO.inverse_mel(mel, nrm, GO.filterbank(cfg["n_fft"], cfg["sample_rate"], cfg["f_min"], cfg["f_max"], cfg["n_mels"], dt))
                for dt in (torch.float32, torch.float64))
    assert float((w64 > 0).float().mean()) > 0.2 and float((w64 == 0).float().mean()) > 0.2       # both sides of the relu
    check(f"inverse_mel {cfg['sample_rate']} norms={with_norms}", got, w32, w64)


@pytest.mark.parametrize("n_iter", [0, 1, 3])
@pytest.mark.parametrize("n_fft,win,hop,F,B", GO.SHAPES)
def test_griffinlim_matches_oracle(engines, n_fft, win, hop, F, B, n_iter):
    n_freq = n_fft // 2 + 1
    S = GO.make_spectrogram(31, B, n_freq, F)
    init = GO.random_angles(32, B, n_freq, F, torch.float32)
    got = engines(n_fft, win, hop).griffinlim(S.to(DEV), init_angles=init.to(DEV), n_iter=n_iter)
    w32 = GO.griffinlim(S, init, n_iter, n_fft, hop, win, dtype=torch.float32)
    w64 = GO.griffinlim(S, init, n_iter, n_fft, hop, win, dtype=torch.float64)
    assert got.shape == (B, hop * (F - 1))
    check(f"griffinlim n_fft={n_fft} win={win} hop={hop} F={F} B={B} n_iter={n_iter}", got, w32, w64)


@pytest.mark.parametrize("n_fft,win,hop,F,B", GO.LONG_SHAPES)
def test_64_iterations(engines, n_fft, win, hop, F, B):
    n_freq = n_fft // 2 + 1
    S = GO.make_spectrogram(41, B, n_freq, F)
    init = GO.random_angles(42, B, n_freq, F, torch.float32)
    got = engines(n_fft, win, hop).griffinlim(S.to(DEV), init_angles=init.to(DEV), n_iter=64)
    w32 = GO.griffinlim(S, init, 64, n_fft, hop, win, dtype=torch.float32)
    w64 = GO.griffinlim(S, init, 64, n_fft, hop, win, dtype=torch.float64)
    sc32, sc64 = (GO.spectral_convergence(w, S, n_fft, hop, win) for w in (w32, w64))
    spread, sc_spread = 0.0, 0.0
    for run in range(4):
        g = torch.Generator().manual_seed(430 + run)
        sign = torch.randint(0, 2, init.shape, generator=g).double() * 2.0 - 1.0
        rot = init.to(torch.complex128) * torch.polar(torch.ones_like(sign), 2.0 ** -22 * sign)
        w = GO.griffinlim(S, rot, 64, n_fft, hop, win, dtype=torch.float64)
        spread = max(spread, float((w - w64).abs().max()))
        sc_spread = max(sc_spread, float((GO.spectral_convergence(w, S, n_fft, hop, win) - sc64).abs().max()))
    print(f"64 iterations n_fft={n_fft} F={F} B={B}: fp32-fp64 {float((w32.double() - w64).abs().max()):.3e}, fp64 spread {spread:.3e}, "
          f"spectral convergence fp32 {sc32.tolist()} fp64 {sc64.tolist()} spread {sc_spread:.3e}")
    check(f"griffinlim 64 n_fft={n_fft} F={F} B={B}", got, w32, w64, extra_floor=spread)
    sc = GO.spectral_convergence(got.cpu(), S, n_fft, hop, win)
    check(f"spectral convergence 64 n_fft={n_fft} F={F} B={B}", sc, sc32, sc64, extra_floor=sc_spread)


def oracle_chain(wav, nrm, cfg, init, n_iter, dtype):
    """forward (utils.py:150-162) then invert, on the CPU"""
    x = wav.to(dtype)
    spec = torch.stft(x, cfg["n_fft"], cfg["hop"], cfg["win"], window=torch.hann_window(cfg["win"], periodic=True, dtype=dtype),
                      center=True, pad_mode="reflect", normalized=False, onesided=True, return_complex=True)
    fb = GO.filterbank(cfg["n_fft"], cfg["sample_rate"], cfg["f_min"], cfg["f_max"], cfg["n_mels"], dtype)
    mel = torch.matmul((spec.real ** 2 + spec.imag ** 2).transpose(1, 2), fb).transpose(1, 2)
    mel = torch.log(torch.clamp(mel, min=1e-5)) / nrm.to(dtype).view(1, -1, 1)
    S = GO.inverse_mel(mel, nrm, fb)
    return GO.griffinlim(S, init, n_iter, cfg["n_fft"], cfg["hop"], cfg["win"], dtype=dtype)


def test_invert_of_forward_end_to_end(norms):
    """a 2048-sample harmonic-plus-noise waveform (F = 9) through the extractor and back, 3 iterations from a given start"""
    from genvc_amd.utils import TorchMelSpectrogram
    cfg = GO.DVAE_MELS[0]
    tm = TorchMelSpectrogram(sampling_rate=cfg["sample_rate"])
    wav = GO.harmonic_noise_wav(51, 1, 2048, cfg["sample_rate"])
    init = GO.random_angles(52, 1, 513, 9, torch.float32)
    mel = tm(wav.to(DEV))
    assert mel.shape == (1, 80, 9)
    got = tm.invert(mel, n_iter=3, init_angles=init.to(DEV))
    assert got.is_cuda and got.shape == (1, 2048) and got.squeeze().cpu().numpy().shape == (2048,)
    w32, w64 = (oracle_chain(wav, norms, cfg, init, 3, dt) for dt in (torch.float32, torch.float64))
    check("invert(forward(wav))", got, w32, w64)
    tm._gl_engine.close()


@pytest.fixture(scope="module")
def extractor():
    from genvc_amd.utils import TorchMelSpectrogram
    tm = TorchMelSpectrogram(sampling_rate=24000)
    yield tm
    if tm._gl_engine is not None:
        tm._gl_engine.close()


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else torch.view_as_real(t).contiguous().view(torch.int32)


def test_determinism_and_the_seeded_start(extractor, norms):
    B, F = 2, 9
    g = torch.Generator().manual_seed(61)
    mel = ((torch.rand(B, 80, F, generator=g) * 8.0 - 9.0) / norms.view(1, -1, 1)).to(DEV)
    a = extractor.invert(mel, n_iter=5, seed=7)
    b = extractor.invert(mel, n_iter=5, seed=7)
    assert a.shape == (B, 256 * (F - 1)) and bool(torch.isfinite(a).all())
    assert torch.equal(bits(a), bits(b))                                                  # two calls, the same bits
    eng = extractor._gl_engine
    init = eng.init_angles(7, B, F)
    assert init.shape == (B, 513, F) and init.dtype == torch.complex64
    assert torch.equal(bits(extractor.invert(mel, n_iter=5, init_angles=init)), bits(a))  # the seed is that start
    c = extractor.invert(mel, n_iter=5, seed=8)
    assert float((c - a).abs().max()) > 1e-3 * float(a.abs().max())                       # another seed, another waveform
    # unit phasors: both components are rounded once from double, so the modulus is 1 to within an fp32 ulp
    z = init.cpu().to(torch.complex128)
    assert float((z.abs() - 1.0).abs().max()) <= 2.0 ** -23
    # uniform phases: mean real and imaginary parts within 5 standard errors (each has variance 1/2) of 0
    n = z.numel()
    se = (0.5 / n) ** 0.5
    print(f"init angles: mean re {float(z.real.mean()):.3e}, mean im {float(z.imag.mean()):.3e}, standard error {se:.3e} over {n}")
    assert abs(float(z.real.mean())) <= 5 * se and abs(float(z.imag.mean())) <= 5 * se
    assert len(torch.unique(z.real)) > 0.9 * n                                            # no two-valued or repeated stream
    # keyed by (seed, item, bin, frame): an entry does not depend on how many items or frames the call has
    assert torch.equal(bits(eng.init_angles(7, 1, F)), bits(init[:1]))
    assert torch.equal(bits(eng.init_angles(7, B, 5)), bits(init[:, :, :5]))
    assert not torch.equal(bits(init[0]), bits(init[1]))


def test_capacity_regrows_the_engine():
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import GriffinLimEngine
    from genvc_amd.utils import TorchMelSpectrogram
    B, F = 2, 9
    g = torch.Generator().manual_seed(71)
    mel = (torch.rand(B, 80, F, generator=g) * 2.0 - 1.0).to(DEV)
    small = TorchMelSpectrogram(sampling_rate=24000, mel_norm_file=None).bind_invert(max_batch=1, max_frames=4)
    assert (small._gl_engine.max_batch, small._gl_engine.max_frames) == (1, 4)
    got = small.invert(mel, n_iter=3, seed=1)
    assert small._gl_engine.max_batch >= B and small._gl_engine.max_frames >= F
    roomy = TorchMelSpectrogram(sampling_rate=24000, mel_norm_file=None).bind_invert(max_batch=4, max_frames=32)
    assert torch.equal(bits(roomy.invert(mel, n_iter=3, seed=1)), bits(got))
    small._gl_engine.close()
    roomy._gl_engine.close()
    # the library itself refuses a call beyond its capacity
    eng = GriffinLimEngine(None, sample_rate=24000, max_batch=1, max_frames=4)
    try:
        S = torch.ones(1, 513, F, device=DEV)
        with pytest.raises(GenvcHipError, match="capacity") as ei:
            eng.griffinlim(S, n_iter=0)
        assert ei.value.code == -1
        assert eng.griffinlim(S[:, :, :4].contiguous(), n_iter=0).shape == (1, 768)
    finally:
        eng.close()


def test_audition_codes():
    """on the tiny acoustic config: invert(decode(codes)), bit for bit, hop (F - 1) samples"""
    from genvc_amd import config as gcfg
    from genvc_amd.inference.model_init import model_init_synthetic
    m, _ = model_init_synthetic(gcfg.default_config(tiny=True, with_acoustic=True), seed=3, device=DEV, max_slots=2)
    g = torch.Generator().manual_seed(81)
    codes = torch.randint(0, int(m.config.acoustic_dvae_config.num_tokens), (2, 5), generator=g).to(DEV)
    wav = m.audition_codes(codes, n_iter=4, seed=2)
    mel = m.acoustic_dvae.decode(codes)[0]
    F = mel.shape[-1]
    assert F == 20 and wav.shape == (2, 256 * (F - 1)) and wav.is_cuda and bool(torch.isfinite(wav).all())
    assert float(wav.abs().max()) > 0.0
    assert torch.equal(bits(m.torch_mel_spectrogram_dvae.invert(mel, n_iter=4, seed=2)), bits(wav))
