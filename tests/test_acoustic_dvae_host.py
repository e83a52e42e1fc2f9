"""Host-side checks of the acoustic DiscreteVAE work (no GPU): the CPU restatement of decode / forward with the polyphase fold
against the reference's own outputs (tests/golden/acoustic_dvae_*.npz), the state-dict key sets, format_batch_on_device's host
arithmetic on stub engines, the refusals, and the declared symbols."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dvae_full_oracle as DO      # noqa: E402
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth        # noqa: E402
from genvc_amd.layers.dvae import DiscreteVAE      # noqa: E402

CFG = {"tiny": DO.TINY, "full": DO.FULL}
DECODE = {"tiny": [(1, 1), (1, 2), (2, 5), (3, 33), (1, 71)], "full": [(1, 24), (2, 71)]}
PRE_STEP = {"tiny": 1, "full": 8}


def make(cfg, **kw):
    return DiscreteVAE(channels=cfg["num_channels"], normalization=None, positional_dims=1, num_tokens=cfg["num_tokens"],
                       codebook_dim=cfg["codebook_dim"], hidden_dim=cfg["hidden_dim"], num_resnet_blocks=cfg["num_resnet_blocks"],
                       kernel_size=cfg["kernel_size"], num_layers=cfg["num_layers"], use_transposed_convs=False, **kw)


@pytest.fixture(scope="module", params=["tiny", "full"])
def case(request, gold):
    tag = request.param
    g = gold(f"acoustic_dvae_{tag}")
    w = synth.make_weights(int(g["seed"]), synth.dvae_full_weight_spec(CFG[tag], codebook_scale=DO.CODEBOOK_SCALE))
    return tag, g, w


def test_oracle_decode_matches_reference(case):
    tag, g, w = case
    codes_seen = set()
    for B, n in DECODE[tag]:
        codes = DO.designed_codes(int(g["seed"]), B, n, CFG[tag]["num_tokens"])
        codes_seen |= set(codes.flatten().tolist())
        out, pre = DO.decode(w, CFG[tag], codes)
        np.testing.assert_allclose(out.numpy(), g[f"dec_out_{B}_{n}"], atol=1e-5, rtol=0)
        np.testing.assert_allclose(pre.numpy()[:, ::PRE_STEP[tag]], g[f"dec_pre_{B}_{n}"], atol=1e-5, rtol=0)
        assert bool((codes[:, 1:] == codes[:, :-1]).any()) or n < 8           # repeated neighbours
    assert 0 in codes_seen and CFG[tag]["num_tokens"] - 1 in codes_seen


def test_oracle_forward_matches_reference(case):
    from genvc_amd.utils import DEFAULT_MEL_NORM_FILE, load_mel_norms
    tag, g, w = case
    B, _, T = g["fwd_out"].shape
    norms = torch.from_numpy(load_mel_norms(DEFAULT_MEL_NORM_FILE))
    feat = DO.mel_1024(DO.acoustic_wavs(int(g["seed"]), "fwd", (T - 1) * 256 + 80, B), norms)
    recon, commit, out, codes = DO.forward(w, CFG[tag], feat)
    assert np.array_equal(codes.numpy(), g["fwd_codes"])
    np.testing.assert_allclose(out.numpy(), g["fwd_out"], atol=1e-5, rtol=0)
    assert abs(float(recon) - float(g["fwd_recon"])) <= 1e-6 and abs(float(commit) - float(g["fwd_commit"])) <= 1e-6
    assert float(g["fwd_margin"].min()) > 1e-4


def test_fixture_screens(case):
    tag, g, _ = case
    n_all = n_safe = 0
    for n in (6000, 24077, 72000):
        assert len(np.unique(g[f"tok_codes_{n}"])) >= 6
        m = g[f"tok_margin_{n}"]
        n_all += m.size; n_safe += int((m > 1e-4).sum())
    assert n_safe >= 0.97 * n_all


def test_fold_is_the_upsampled_conv():
    for k, n in ((3, 7), (5, 6), (7, 5), (1, 4)):
        w = synth.uniform(1, f"fold_w{k}", (6, 4, k), 0.3)
        b = synth.uniform(1, f"fold_b{k}", (6,), 0.1)
        x = synth.uniform(1, f"fold_x{k}", (2, 4, n), 1.0)
        ref = torch.relu(torch.nn.functional.conv1d(torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"), w, b,
                                                    padding=(k - 1) // 2))
        np.testing.assert_allclose(DO.upconv_polyphase(x, w, b).numpy(), ref.numpy(), atol=1e-6, rtol=0)
        assert all(wf.shape[-1] == (k - 1) // 2 + 1 for _, wf in DO.fold_upconv(w))


def test_state_dict_keys(case):
    tag, g, w = case
    c = gcfg.DEFAULT_CONTENT_DVAE
    plain = DiscreteVAE(channels=c["num_channels"], normalization=None, positional_dims=1, num_tokens=c["num_tokens"],
                        codebook_dim=c["codebook_dim"], hidden_dim=c["hidden_dim"], num_resnet_blocks=c["num_resnet_blocks"],
                        kernel_size=c["kernel_size"], num_layers=c["num_layers"], use_transposed_convs=False)
    assert sorted(plain.state_dict()) == sorted(synth.dvae_weight_spec(c))            # a content DVAE built as before: unchanged
    assert not any(k.startswith("decoder.") for k in plain.state_dict())
    full = make(CFG[tag], with_decoder=True)
    assert sorted(full.state_dict()) == sorted(g["keys"].tolist())
    assert sorted(w) == sorted(g["keys"].tolist())
    missing, unexpected = full.load_state_dict(w, strict=True)
    assert not missing and not unexpected
    # the "codebook" kind and the encoder-only spec are what they were
    assert torch.equal(synth.make_weights(7, synth.dvae_weight_spec(c))["codebook.embed"], synth.uniform(7, "codebook.embed", (512, 256), 1.0))


def test_no_resblocks_decoder_layout():
    cfg = dict(DO.TINY, num_resnet_blocks=0)
    m = make(cfg, with_decoder=True)
    keys = sorted(k for k in m.state_dict() if k.startswith("decoder."))
    assert keys == sorted(f"decoder.{i}.0.conv.{p}" for i in (0, 1) for p in ("weight", "bias")) + ["decoder.2.bias", "decoder.2.weight"]
    assert m.state_dict()["decoder.0.0.conv.weight"].shape == (64, 64, 3)             # the first stage reads codebook_dim channels
    assert sorted(m.state_dict()) == sorted(synth.dvae_full_weight_spec(cfg))


def test_refusals():
    m = make(DO.TINY, with_decoder=True)
    assert m.training
    with pytest.raises(NotImplementedError, match="training"):
        m(torch.zeros(1, 80, 8))
    m.eval()
    with pytest.raises(ValueError, match="multiple of 4"):
        m(torch.zeros(1, 80, 10))
    for bad in (1024, -1):
        with pytest.raises(ValueError, match="codes"):
            m.decode(torch.tensor([[3, bad, 5]]))
    plain = make(DO.TINY).eval()
    for call in (lambda: plain.decode(torch.zeros(1, 4, dtype=torch.long)), lambda: plain.infer(torch.zeros(1, 80, 8)),
                 lambda: plain(torch.zeros(1, 80, 8))):
        with pytest.raises(NotImplementedError, match="decoder"):
            call()
    with pytest.raises(NotImplementedError):
        DiscreteVAE(positional_dims=2, with_decoder=True)           # 2-D DVAEs stay out of scope


class _Stub(torch.nn.Module):
    """stands in for an extractor / engine-backed module: records the shapes it is given, returns zeros of the right shape"""

    def __init__(self, fn):
        super().__init__()
        self.fn, self.calls = fn, []

    def forward(self, x, *a, **k):
        self.calls.append(tuple(x.shape))
        return self.fn(x)

    extract_content_features = get_codebook_indices = forward


def _stub_model(monkeypatch, **cfg_over):
    from genvc_amd.inference import model_init as MI
    cfg = gcfg.default_config(tiny=True, with_acoustic=True)
    for k, v in cfg_over.items():
        cfg[k] = v
    m = MI.GenVCModel(cfg)
    m.torch_mel_spectrogram_style_encoder = _Stub(lambda x: torch.zeros(x.shape[0], 80, 1 + x.shape[-1] // 256))
    m.torch_mel_spectrogram_dvae = _Stub(lambda x: torch.zeros(x.shape[0], 80, 1 + x.shape[-1] // 256))
    m.acoustic_dvae = _Stub(lambda x: torch.zeros(x.shape[0], (x.shape[-1] + 3) // 4, dtype=torch.long))
    m.content_extractor = _Stub(lambda x: torch.zeros(x.shape[0], (x.shape[-1] - 400) // 320 + 1, 256))
    m.content_dvae = _Stub(lambda x: torch.zeros(x.shape[0], (x.shape[-1] + 3) // 4, dtype=torch.long))
    res = _Stub(lambda x: torch.zeros(x.shape[0], -(-x.shape[-1] * 2 // 3)))
    monkeypatch.setattr(MI, "resample", lambda x, a, b: res(x) if (a, b) == (24000, 16000) else None)
    return m, res


def test_format_batch_host_arithmetic(monkeypatch):
    from genvc_amd.inference.model_init import content_pad_samples, default_text_lengths
    m, res = _stub_model(monkeypatch)
    batch = dict(wav=torch.zeros(2, 1, 24000), wav_lengths=torch.tensor([24000, 14400]), conditioning=torch.zeros(2, 3, 1, 12000),
                 cond_lens=torch.tensor([12000, 9000]))
    b = m.format_batch_on_device(batch)
    assert m.torch_mel_spectrogram_style_encoder.calls == [(6, 1, 12000)] and b["cond_mels"].shape == (2, 3, 80, 47)
    assert m.torch_mel_spectrogram_dvae.calls == [(2, 1, 24000)] and m.acoustic_dvae.calls == [(2, 80, 94)]
    assert b["audio_codes"].shape == (2, 24)
    assert res.calls == [(2, 24000)]
    assert m.content_extractor.calls == [(2, 16000 + 320)]                    # int(0.02 * 16000) zero samples appended
    assert m.content_dvae.calls == [(2, 256, 50)] and b["text_inputs"].shape == (2, 13)
    assert b["text_lengths"].tolist() == [12, 7] and b["text_lengths"].dtype == torch.long     # // (int(0.02 * 24000) * 4)
    assert content_pad_samples(0.02, 16000) == 320 and default_text_lengths([1919, 1920, 3840], 24000).tolist() == [0, 1, 2]
    # given text_lengths are kept (as long); another text_frame_rate changes the padding and the default
    b2 = m.format_batch_on_device(dict(batch, text_lengths=torch.tensor([5, 4], dtype=torch.int32)))
    assert b2["text_lengths"].tolist() == [5, 4] and b2["text_lengths"].dtype == torch.long
    m2, _ = _stub_model(monkeypatch, text_frame_rate=0.04)
    b3 = m2.format_batch_on_device(dict(batch, text_lengths=None))
    assert m2.content_extractor.calls == [(2, 16000 + 640)] and b3["text_lengths"].tolist() == [6, 3]


def test_format_batch_refusals(monkeypatch):
    from genvc_amd.inference.model_init import GenVCModel
    batch = dict(wav=torch.zeros(1, 1, 24000), wav_lengths=torch.tensor([24000]), conditioning=torch.zeros(1, 1, 1, 12000),
                 cond_lens=torch.tensor([12000]))
    plain = GenVCModel(gcfg.default_config(tiny=True))
    assert plain.acoustic_dvae is None and not any(k.startswith("acoustic_dvae.") for k in plain.state_dict())
    with pytest.raises(NotImplementedError, match="acoustic_dvae_config"):
        plain.format_batch_on_device(dict(batch))
    cfg = gcfg.default_config(tiny=True, with_acoustic=True)
    cfg.acoustic_dvae_config["dvae_sample_rate"] = 22050
    with pytest.raises(NotImplementedError, match="22050"):
        GenVCModel(cfg).format_batch_on_device(dict(batch))


def test_default_config_is_unchanged_and_acoustic_is_opt_in():
    assert "acoustic_dvae_config" not in gcfg.default_config() and "acoustic_dvae_config" not in gcfg.default_config(tiny=True)
    a = gcfg.default_config(with_acoustic=True).acoustic_dvae_config
    assert {k: a[k] for k in DO.FULL} == DO.FULL and a.dvae_sample_rate == 24000
    from genvc_amd.inference.model_init import _REQUIRED_PREFIXES
    assert "acoustic_dvae." not in _REQUIRED_PREFIXES


def test_new_symbols_are_declared():
    from genvc_amd import _lib
    header = open(os.path.join(DO.ROOT, "include", "genvc_hip.h")).read()
    for name in ("gvc_dvae_create_ex", "gvc_dvae_decode", "gvc_dvae_code_error", "gvc_dvae_reconstruct"):
        assert name in _lib.exported_symbols() and f"int {name}(" in header
    assert "#define GVC_DVAE_DECODER 1" in header and _lib.DVAE_DECODER == 1
