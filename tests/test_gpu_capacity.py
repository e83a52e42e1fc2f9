"""GPU parity of the vocoder and the encoders at the capacities they are bound with by default: HifiganEngine 2 x 2560 frames,
DvaeEngine 8 x 1504, HubertEngine 2 x 480 000 samples, PerceiverEngine 8 x 2816.  The shapes sit on either side of every
code-path switch that only a long call reaches (conv_pre off the K-split kernel past B x T0 = 1024, the DVAE off the
one-round-trip conv kernel past B x T = 600), at the capacity itself, and one step beyond it (refused on the host).

Every case is compared with the float64 oracle of the same inputs under act_stats.yardstick: the kernel's largest deviation
must stay within the larger of 8x the float32 oracle's own deviation on that case and 4x the kernel's deviation on a short
shape of the same weights that the golden tests already cover (the "tame" pair), plus 1e-6 max|ref|.  The tame pair itself is
held to the first term alone.  A failure names the batch item, frame and channel of the largest deviation.  Run with -s: one yardstick line per case, and the device memory in use."""
import numpy as np
import pytest
import torch

import act_stats as A
from genvc_amd import config as gcfg
from genvc_amd import synth
from oracle import genvc_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

_MEM0 = [0]


def _mem(tag=None):
    """device memory in use (engines allocate outside torch's pool); without a tag: the baseline the next lines are relative to"""
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if tag is None:
        _MEM0[0] = total - free
    else:
        print(f"device memory, {tag}: +{(total - free - _MEM0[0]) / 2 ** 30:.2f} GiB (in use on the device: {(total - free) / 2 ** 30:.2f} GiB)")


def _where(kern, ref64, axes):
    """the element of the largest deviation, e.g. 'item 1, frame 1203, channel 77'; an axis named 'sample' also gets its frame"""
    d = (kern.detach().cpu().double() - ref64.double()).abs()
    idx = np.unravel_index(int(d.argmax()), tuple(d.shape))
    parts = []
    for name, i in zip(axes, idx):
        if name is None:
            continue
        parts.append(f"{name} {int(i)}")
        if name == "sample":
            parts.append(f"frame {int(i) // 256}")
    return ", ".join(parts) + f" (kernel {float(kern.detach().cpu()[idx]):.6g}, float64 {float(ref64[idx]):.6g})"


def _check(name, kern, ref64, ref32, tame, axes):
    """act_stats.yardstick with the location of the largest deviation added to a failure; tame = (kernel, float64) of the short shape"""
    assert tuple(kern.shape) == tuple(ref64.shape), f"{name}: shape {tuple(kern.shape)} != {tuple(ref64.shape)}"
    assert bool(torch.isfinite(kern).all()), f"{name}: non-finite output"
    try:
        return A.yardstick(name, kern.cpu(), ref64, ref32, tame[0], tame[1])
    except AssertionError as e:
        raise AssertionError(f"{e}; largest deviation at {_where(kern, ref64, axes)}") from None


def _tame(name, kern, ref64, ref32, axes):
    """the short shape of the same weights, whose deviation is the yardstick's second term.  That term only means something if the short
    shape is itself right (an error that a path makes at every length would otherwise widen its own bound), so the pair is held to
    the first term alone: 8x the float32 oracle's deviation + 1e-6 max|ref| (the yardstick with a tame deviation of zero)"""
    _check(name + " (tame pair)", kern, ref64, ref32, (ref64, ref64), axes)
    return kern.cpu(), ref64


# ---------------------------------------------------------------------------
# vocoder
# ---------------------------------------------------------------------------

WAV_AXES = ("item", None, "sample")
_VOC = {}            # (config tag, seed, B, n) -> (latents, float64 wav, float32 wav): the modes below share the oracle runs


def _voc_weights(tag, seed):
    c = gcfg.DEFAULT_VOCODER if tag == "full" else gcfg.TINY_VOCODER
    return c, synth.make_weights(seed, synth.hifigan_weight_spec(c))


def _voc_case(tag, seed, B, n, want32=True):
    key = (tag, seed, B, n)
    if key not in _VOC:
        c, w = _voc_weights(tag, seed)
        lat = synth.uniform(seed, f"lat_{B}_{n}", (B, n, c["input_feat_dim"]), 1.0)
        r64 = O.vocode_latents(A.double(w), c, lat.double())
        peak = float(r64.abs().max())
        # tanh must not saturate: it would flatten an error of the layers in front of it
        assert peak < 0.99, f"vocoder {tag} {B}x{n}: the float64 waveform reaches {peak:.3f}"
        _VOC[key] = [lat, r64, None]
    if want32 and _VOC[key][2] is None:
        c, w = _voc_weights(tag, seed)
        _VOC[key][2] = O.vocode_latents(w, c, _VOC[key][0])
    return _VOC[key]


def _voc_engine(tag, seed, **cap):
    from genvc_amd.engine import HifiganEngine
    c, w = _voc_weights(tag, seed)
    eng = HifiganEngine(c, **cap)                                   # default capacity: 2 x 2560 frames
    eng.bind({k: v.to(DEV) for k, v in w.items()})
    return eng


def _voc_tame(eng, tag, seed):
    lat, r64, r32 = _voc_case(tag, seed, 1, 8)
    return _tame(f"vocoder {tag} 1x8 latents", eng.forward_latents(lat.to(DEV), 4), r64, r32, WAV_AXES)


VOC_SEED = 21


def test_vocoder_trained_configuration_up_to_capacity():
    """one engine of 2 x 2560 frames, (B, latents) in an order that changes the geometry on every call but the first (the tame pair
    is the same 1 x 8 call, so the loop's first call already replays its graph): 256 / 257 latents and
    2 x 128 / 2 x 129 sit either side of B x T0 = 1024 frames, where conv_pre leaves the K-split kernel for the tiled GEMM
    (hifigan.hip hf_body); 640 latents = 2560 frames is the capacity (655 360 frames of 32 channels in the last stage).  Both entry
    points at (1, 257) and (1, 640).  The second (1, 8) and (1, 257) replay a cached graph after other geometries ran."""
    _mem()
    eng = _voc_engine("full", VOC_SEED)
    _mem("vocoder 2 x 2560 bound")
    tame = _voc_tame(eng, "full", VOC_SEED)
    first = {}
    for B, n in ((1, 8), (1, 256), (1, 257), (2, 128), (2, 129), (1, 640), (1, 8), (2, 640), (1, 257)):
        lat, r64, r32 = _voc_case("full", VOC_SEED, B, n)
        got = eng.forward_latents(lat.to(DEV), 4).cpu()
        if (B, n) in first:
            assert torch.equal(got, first[(B, n)]), f"vocoder {B}x{n}: the replay differs from the first call at {_where(got, first[(B, n)], WAV_AXES)}"
        else:
            first[(B, n)] = got
        _check(f"vocoder {B}x{n} latents ({4 * n} frames)", got, r64, r32, tame, WAV_AXES)
        if (B, n) in ((1, 257), (1, 640)):
            mel = torch.nn.functional.interpolate(lat.transpose(1, 2), scale_factor=[4.0], mode="linear").contiguous()
            _check(f"vocoder {B}x{n} channels-first entry", eng.forward(mel.to(DEV)).cpu(), r64, r32, tame, WAV_AXES)
    _mem("vocoder after 2 x 2560 frames")
    eng.close()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("env", [("GVC_VOCODER_SMALL_CONV", "0"), ("GVC_VOCODER_SMALL_CONV", "2"), ("GVC_VOCODER_GRAPH", "0")],
                         ids=["small_conv_0", "small_conv_2", "graph_0"])
def test_vocoder_fallback_modes_at_length(monkeypatch, env):
    """the paths behind GVC_VOCODER_SMALL_CONV (0: every conv on the tiled GEMM, running ResBlock sum; 2: ResBlock planes added by
    k_sum_planes for a tiled-GEMM upsampling layer) and the launch-per-call path (GVC_VOCODER_GRAPH=0) past B x T0 = 1024;
    mode 0 also at the capacity, where the last stage's GEMMs have 655 360 rows"""
    monkeypatch.setenv(*env)
    eng = _voc_engine("full", VOC_SEED)
    tame = _voc_tame(eng, "full", VOC_SEED)
    for B, n in ((1, 257), (2, 129)) + (((1, 640),) if env == ("GVC_VOCODER_SMALL_CONV", "0") else ()):
        lat, r64, r32 = _voc_case("full", VOC_SEED, B, n)
        _check(f"vocoder {env[0]}={env[1]} {B}x{n} latents", eng.forward_latents(lat.to(DEV), 4).cpu(), r64, r32, tame, WAV_AXES)
    eng.close()
    torch.cuda.empty_cache()


def test_vocoder_graph_cache_eviction():
    """the graph cache drops all its plans when it holds 64 (hifigan.hip hf_run): 70 calls with 70 latent counts, the first five
    again (re-captured: they were dropped), every result against the oracle and the repeats bit for bit; then calls without a
    host sync across an eviction, so that plans are destroyed while launches of theirs may be in flight"""
    seed = 21
    eng = _voc_engine("tiny", seed)
    tame = _voc_tame(eng, "tiny", seed)
    first = {}

    def call(n):
        lat, r64, r32 = _voc_case("tiny", seed, 1, n)
        got = eng.forward_latents(lat.to(DEV), 4)
        if n in first:
            assert torch.equal(got.cpu(), first[n]), f"vocoder graph cache, {n} latents: the repeat differs at {_where(got, first[n], WAV_AXES)}"
        else:
            first[n] = got.cpu()
        _check(f"vocoder tiny 1x{n} latents", got, r64, r32, tame, WAV_AXES)

    for n in list(range(1, 71)) + [1, 2, 3, 4, 5]:
        call(n)
    # call 65 dropped the plans of 1..64, so the cache now holds 65..70 and 1..5: 11 plans.  53 more (6..58, all dropped before)
    # bring it to 64, so that the next shape it does not hold evicts
    for n in range(6, 59):
        call(n)
    order = (1, 2, 59, 1, 2, 60, 59, 1)                            # 59 evicts while 1 and 2 are in flight; 1, 2 and 60 are captured anew
    lats = {n: _voc_case("tiny", seed, 1, n)[0].to(DEV) for n in set(order)}
    torch.cuda.synchronize()
    outs = [eng.forward_latents(lats[n], 4) for n in order]        # no sync in between
    torch.cuda.synchronize()
    for i, (n, wav) in enumerate(zip(order, outs)):
        assert torch.equal(wav.cpu(), first[n]), f"back-to-back call {i} ({n} latents) differs at {_where(wav, first[n], WAV_AXES)}"
    eng.close()
    torch.cuda.empty_cache()


def test_vocoder_windows_at_the_default_capacity():
    """HiFiGAN.bind() with its defaults, trained configuration, 700 latents = 2800 frames: two overlapping windows (2528 and 336
    frames) against the one-shot oracle -- the shape of every call a long conversion makes"""
    from genvc_amd.layers.hifigan import HiFiGAN
    c, w = _voc_weights("full", VOC_SEED)
    v = HiFiGAN(c["input_feat_dim"], c["upsample_initial_channel"], c["resblock_kernel_sizes"], c["resblock_dilation_sizes"],
                c["upsample_rates"], c["upsample_kernel_sizes"], resblock_type="2")
    v.load_state_dict(w)
    v.to(DEV).bind()
    assert v._engine.max_frames == 2560
    lat8, t64, t32 = _voc_case("full", VOC_SEED, 1, 8)
    tame = _tame("vocoder module 1x8 latents", v.forward_latents(lat8.to(DEV), 4), t64, t32, WAV_AXES)
    lat, r64, r32 = _voc_case("full", VOC_SEED, 1, 700)
    _check("vocoder windows 1x700 latents (2800 frames)", v.forward_latents(lat.to(DEV), 4).cpu(), r64, r32, tame, WAV_AXES)
    v._engine.close()
    del v
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# DVAE
# ---------------------------------------------------------------------------

ENC_AXES = ("item", "frame", "channel")
DVAE_SEED = 31


def _dvae_case(w, w64, B, T):
    c = gcfg.DEFAULT_CONTENT_DVAE
    feat = synth.uniform(DVAE_SEED, f"feat_{B}_{T}", (B, c["num_channels"], T), 1.0)
    r64 = O.dvae_encode(w64, feat.double())
    return feat, r64, O.dvae_encode(w, feat)


def _dvae_codes(name, codes, r64, embed64):
    """codes equal the float64 decision on every frame whose float64 top-1 / top-2 distance margin exceeds 1e-3; >= 97 % do"""
    flat = r64.reshape(-1, r64.shape[-1])
    dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ embed64 + embed64.pow(2).sum(0, keepdim=True)
    top2 = (-dist).topk(2, dim=1).values
    safe = ((top2[:, 0] - top2[:, 1]) > 1e-3).view(r64.shape[:-1])
    exp = O.vq_indices(r64, embed64)
    got = codes.cpu().long()
    assert got.shape == exp.shape
    bad = safe & (got != exp)
    print(f"{name}: {int(safe.sum())}/{safe.numel()} frames with a float64 margin > 1e-3, {int(bad.sum())} of them differ")
    assert float(safe.double().mean()) >= 0.97, f"{name}: only {float(safe.double().mean()):.3f} of the frames pass the margin screen"
    if bool(bad.any()):
        b, t = [int(i) for i in bad.nonzero()[0]]
        raise AssertionError(f"{name}: {int(bad.sum())} codes differ from float64 at a clear margin, first at item {b}, frame {t}: "
                             f"{int(got[b, t])} != {int(exp[b, t])}")


def test_dvae_trained_configuration_up_to_capacity():
    """engine 8 x 1504: 8 x 75 = 600 frames is the last shape on the one-round-trip conv kernel and 8 x 76 the first on the
    tiled GEMM (dvae.hip dvae_run), likewise 2 x 300 / 2 x 301; 8 x 299 is an offline batch of 6 s segments, 8 x 1504 the capacity"""
    from genvc_amd.engine import DvaeEngine
    c = gcfg.DEFAULT_CONTENT_DVAE
    w = synth.make_weights(DVAE_SEED, synth.dvae_weight_spec(c))
    w64 = A.double(w)
    _mem()
    eng = DvaeEngine(c)                                             # default capacity: 8 x 1504
    eng.bind({k: v.to(DEV) for k, v in w.items()})
    _mem("DVAE 8 x 1504 bound")
    feat, t64, t32 = _dvae_case(w, w64, 2, 299)
    tame = _tame("DVAE 2x299 enc", eng.encode(feat.to(DEV), return_enc=True)[1], t64, t32, ENC_AXES)
    for B, T in ((8, 75), (8, 76), (2, 300), (2, 301), (8, 299), (1, 1504), (8, 1504), (1, 49)):
        feat, r64, r32 = _dvae_case(w, w64, B, T)
        codes, enc = eng.encode(feat.to(DEV), return_enc=True)
        _check(f"DVAE {B}x{T} enc", enc, r64, r32, tame, ENC_AXES)
        _dvae_codes(f"DVAE {B}x{T} codes", codes, r64, w64["codebook.embed"])
        if (B, T) in ((8, 299), (8, 75)):                           # staged by a strided copy instead of the transpose kernel
            codes_f, enc_f = eng.encode(feat.transpose(1, 2).contiguous().to(DEV), return_enc=True, frames_major=True)
            _check(f"DVAE {B}x{T} enc (frames-major input)", enc_f, r64, r32, tame, ENC_AXES)
            _dvae_codes(f"DVAE {B}x{T} codes (frames-major input)", codes_f, r64, w64["codebook.embed"])
    eng.close()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# ContentVec
# ---------------------------------------------------------------------------

FEAT_AXES = ("item", "frame", "channel")
HUBERT_SEED = 17


def _hubert_wav(B, T):
    return torch.cat([synth.synth_audio(HUBERT_SEED + b, f"wav{T}", T) for b in range(B)], 0)


def test_contentvec_trained_configuration_up_to_capacity():
    """engine 2 x 480 000 samples (30 s): 1499-frame attention and GEMMs, the positional conv at utterance length, GroupNorm
    statistics over 96 000 frames of the first conv layer; then a short call again.  One 30 s input with 2 s of digital
    silence in the middle and a zero tail of 1 s: about 150 padding frames, masked out of 1499 keys"""
    from genvc_amd.engine import HubertEngine
    c = gcfg.DEFAULT_HUBERT
    w = synth.make_weights(HUBERT_SEED, synth.hubert_weight_spec(c))
    w64 = A.double(w)
    _mem()
    eng = HubertEngine(c)                                           # default capacity: 2 x 480 000
    eng.bind({k: v.to(DEV) for k, v in w.items()})
    _mem("ContentVec 2 x 480 000 bound")
    wav = _hubert_wav(1, 16000)
    tame = _tame("ContentVec 1x16000 features", eng.forward(wav.to(DEV)), O.hubert_extract_features(w64, c, wav.double()),
                 O.hubert_extract_features(w, c, wav), FEAT_AXES)
    for B, T in ((1, 480000), (2, 96000), (2, 480000), (1, 16000)):
        wav = _hubert_wav(B, T)
        r64 = O.hubert_extract_features(w64, c, wav.double())
        r32 = O.hubert_extract_features(w, c, wav)
        _check(f"ContentVec {B}x{T} features", eng.forward(wav.to(DEV)), r64, r32, tame, FEAT_AXES)
    wav = _hubert_wav(1, 480000).clone()
    wav[:, 224000:256000] = 0.0
    wav[:, -16000:] = 0.0
    n_pad = int(O.hubert_frame_padding_mask(wav, eng.frames(480000)).sum())
    assert eng.frames(480000) == 1499 and n_pad >= 140, n_pad
    r64 = O.hubert_extract_features(w64, c, wav.double())
    r32 = O.hubert_extract_features(w, c, wav)
    assert A.maxdev(O.hubert_extract_features(w, c, wav, padding_mask=False), r64) > 1e-2        # the mask matters
    _check(f"ContentVec 1x480000 with {n_pad} padding frames", eng.forward(wav.to(DEV)), r64, r32, tame, FEAT_AXES)
    _mem("ContentVec after 2 x 480 000")
    eng.close()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# Perceiver
# ---------------------------------------------------------------------------

LAT_AXES = ("item", "latent", "channel")
PERC = dict(dim=1024, depth=4, dim_context=80, num_latents=32, dim_head=64, heads=8, ff_mult=4)
PERC_SEED = 5


def _perc_weights():
    return synth.make_weights(1, synth.perceiver_weight_spec(1024, prefix="conditioning_perceiver."))


def _perc_case(w, w64, B, Fr):
    x = synth.uniform(PERC_SEED, f"mel_{B}_{Fr}", (B, 80, Fr), 1.0).permute(0, 2, 1).contiguous()
    return x, O.perceiver_forward(w64, x.double()), O.perceiver_forward(w, x)


def test_perceiver_trained_width_up_to_capacity():
    """engine 8 x 2816 frames: more than 2 items beyond 100 frames, the context projection at 8 x 2816 rows"""
    from genvc_amd.engine import PerceiverEngine
    w = _perc_weights()
    w64 = A.double(w)
    _mem()
    eng = PerceiverEngine(**PERC)                                   # default capacity: 8 x 2816
    eng.bind({k: v.to(DEV) for k, v in w.items()}, prefix="conditioning_perceiver.")
    _mem("Perceiver 8 x 2816 bound")
    x, t64, t32 = _perc_case(w, w64, 2, 563)
    tame = _tame("Perceiver 2x563 latents", eng.forward(x.to(DEV)), t64, t32, LAT_AXES)
    for B, Fr in ((1, 2816), (8, 563), (8, 2816), (5, 600), (1, 282)):
        x, r64, r32 = _perc_case(w, w64, B, Fr)
        _check(f"Perceiver {B}x{Fr} latents", eng.forward(x.to(DEV)), r64, r32, tame, LAT_AXES)
    eng.close()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# one step beyond the capacity
# ---------------------------------------------------------------------------

# One frame or one batch item beyond the bound capacity is refused on the host, before any launch (hifigan.hip hf_prepare, dvae.hip
# dvae_check, the capacity line of gvc_perceiver_forward), and the next call within the capacity still equals the oracle.

def test_vocoder_capacity_is_enforced_not_overrun():
    from genvc_amd._lib import GenvcHipError
    eng = _voc_engine("full", VOC_SEED)
    tame = _voc_tame(eng, "full", VOC_SEED)
    d = gcfg.DEFAULT_VOCODER["input_feat_dim"]
    for B, n in ((1, 641), (3, 8), (3, 640)):
        with pytest.raises(GenvcHipError):
            eng.forward_latents(torch.zeros(B, n, d, device=DEV), 4)
    for B, T in ((1, 2561), (3, 32)):
        with pytest.raises(GenvcHipError):
            eng.forward(torch.zeros(B, d, T, device=DEV))
    lat, r64, r32 = _voc_case("full", VOC_SEED, 2, 129)
    _check("vocoder 2x129 latents after refused calls", eng.forward_latents(lat.to(DEV), 4), r64, r32, tame, WAV_AXES)
    eng.close()
    torch.cuda.empty_cache()


def test_dvae_capacity_is_enforced_not_overrun():
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import DvaeEngine
    c = gcfg.DEFAULT_CONTENT_DVAE
    w = synth.make_weights(DVAE_SEED, synth.dvae_weight_spec(c))
    w64 = A.double(w)
    eng = DvaeEngine(c)
    eng.bind({k: v.to(DEV) for k, v in w.items()})
    feat, t64, t32 = _dvae_case(w, w64, 2, 299)
    tame = _tame("DVAE 2x299 enc", eng.encode(feat.to(DEV), return_enc=True)[1], t64, t32, ENC_AXES)
    for B, T in ((1, 1505), (9, 49), (9, 1504)):
        for fm in (False, True):
            x = torch.zeros((B, T, c["num_channels"]) if fm else (B, c["num_channels"], T), device=DEV)
            with pytest.raises(GenvcHipError):
                eng.encode(x, frames_major=fm)
    feat, r64, r32 = _dvae_case(w, w64, 8, 76)
    codes, enc = eng.encode(feat.to(DEV), return_enc=True)
    _check("DVAE 8x76 enc after refused calls", enc, r64, r32, tame, ENC_AXES)
    _dvae_codes("DVAE 8x76 codes after refused calls", codes, r64, w64["codebook.embed"])
    eng.close()
    torch.cuda.empty_cache()


def test_perceiver_capacity_is_enforced_not_overrun():
    from genvc_amd._lib import GenvcHipError
    from genvc_amd.engine import PerceiverEngine
    w = _perc_weights()
    w64 = A.double(w)
    eng = PerceiverEngine(**PERC)
    eng.bind({k: v.to(DEV) for k, v in w.items()}, prefix="conditioning_perceiver.")
    x, t64, t32 = _perc_case(w, w64, 2, 563)
    tame = _tame("Perceiver 2x563 latents", eng.forward(x.to(DEV)), t64, t32, LAT_AXES)
    for B, Fr in ((1, 2817), (9, 100), (9, 2816)):
        with pytest.raises(GenvcHipError):
            eng.forward(torch.zeros(B, Fr, 80, device=DEV))
    x, r64, r32 = _perc_case(w, w64, 5, 600)
    _check("Perceiver 5x600 latents after refused calls", eng.forward(x.to(DEV)), r64, r32, tame, LAT_AXES)
    eng.close()
    torch.cuda.empty_cache()
