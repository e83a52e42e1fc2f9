"""DiscreteVAE of the reference (/root/reference/layers/dvae.py:203-381, eval mode only) on libgenvc_hip: the content tokenizer
(`get_codebook_indices`, gvc_dvae_encode) and, with the decoder (`with_decoder=True`), the acoustic
DVAE's `decode`, `infer` and eval-mode `forward` (gvc_dvae_decode, gvc_dvae_reconstruct)."""
import torch
from torch import nn

from ..engine import DvaeEngine


class _Holder(nn.Module):
    pass


def _conv(cout, cin, k):
    m = _Holder()
    m.weight = nn.Parameter(torch.empty(cout, cin, k).normal_(std=0.02), requires_grad=False)
    m.bias = nn.Parameter(torch.zeros(cout), requires_grad=False)
    return m


class DiscreteVAE(nn.Module):
    def __init__(self, positional_dims=1, num_tokens=512, codebook_dim=512, num_layers=3, num_resnet_blocks=0,
                 hidden_dim=64, channels=3, stride=2, kernel_size=4, use_transposed_convs=True, encoder_norm=False,
                 activation="relu", normalization=None, with_decoder=False, **_unused):
        super().__init__()
        if positional_dims != 1 or stride != 2 or encoder_norm or activation != "relu" or normalization is not None:
            raise NotImplementedError("only the 1-D, stride-2, ReLU, un-normalised content DVAE of GenVC is supported")
        self.cfg = dict(num_channels=channels, num_tokens=num_tokens, codebook_dim=codebook_dim, hidden_dim=hidden_dim,
                        num_resnet_blocks=num_resnet_blocks, kernel_size=kernel_size, num_layers=num_layers)
        self.num_tokens = num_tokens
        layers = []
        cin = channels
        for i in range(num_layers):
            blk = nn.ModuleList([_conv(hidden_dim * 2 ** i, cin, kernel_size)])      # encoder.{i}.0.*
            layers.append(blk)
            cin = hidden_dim * 2 ** i
        for _ in range(num_resnet_blocks):
            rb = _Holder()
            rb.net = nn.ModuleList([_conv(cin, cin, 3), _Holder(), _conv(cin, cin, 3), _Holder(), _conv(cin, cin, 1)])
            layers.append(rb)                                                          # encoder.{i}.net.{0,2,4}.*
        layers.append(_conv(codebook_dim, cin, 1))                                     # encoder.{last}.*
        self.encoder = nn.ModuleList(layers)
        self.codebook = _Holder()
        self.codebook.register_buffer("embed", torch.randn(codebook_dim, num_tokens))
        self._engine = None
        self.decoder = None
        if with_decoder:
            self._build_decoder()

    def _build_decoder(self):
        """the parameter holders of the reference's decoder with use_transposed_convs=False (dvae.py:252-292), under its key names"""
        c = self.cfg
        hid, nl, k = c["hidden_dim"], c["num_layers"], c["kernel_size"]
        inner = hid * 2 ** (nl - 1)
        layers = []
        cin = c["codebook_dim"]
        if c["num_resnet_blocks"] > 0:
            layers.append(_conv(inner, cin, 1))                                        # decoder.0.*
            cin = inner
        for _ in range(c["num_resnet_blocks"]):
            rb = _Holder()
            rb.net = nn.ModuleList([_conv(cin, cin, 3), _Holder(), _conv(cin, cin, 3), _Holder(), _conv(cin, cin, 1)])
            layers.append(rb)                                                          # decoder.{i}.net.{0,2,4}.*
        for i in range(nl):
            up = _Holder()
            up.conv = _conv(hid * 2 ** (nl - 1 - i), cin, k)
            layers.append(nn.ModuleList([up]))                                         # decoder.{i}.0.conv.*
            cin = hid * 2 ** (nl - 1 - i)
        layers.append(_conv(c["num_channels"], cin, 1))                                # decoder.{last}.*
        self.decoder = nn.ModuleList(layers).to(self.codebook.embed.device)

    def bind(self, max_batch=8, max_frames=1504):
        if self._engine is not None:
            self._engine.close()
        self._engine = DvaeEngine(self.cfg, max_batch=max_batch, max_frames=max_frames, with_decoder=self.decoder is not None)
        self._engine.bind(dict(self.state_dict()))
        return self

    def _require_decoder(self, what):
        if self.decoder is None:
            raise NotImplementedError(f"DiscreteVAE.{what}: this DVAE was built without a decoder (with_decoder=True)")

    def _bound(self):
        if self._engine is None or not self._engine.with_decoder:
            self.bind()
        return self._engine

    @torch.inference_mode()
    def decode(self, img_seq):
        """codes [B,n] -> (out [B,channels,n 2^L], the last layer's input [B,hidden,n 2^L]) (dvae.py:333-352)"""
        self._require_decoder("decode")
        if not img_seq.is_cuda:         # (codes already on the device are checked by the gather kernel: no extra synchronisation)
            if img_seq.numel() and (int(img_seq.min()) < 0 or int(img_seq.max()) >= self.num_tokens):
                raise ValueError(f"DiscreteVAE.decode: codes must lie in [0, {self.num_tokens})")
            img_seq = img_seq.to(self.codebook.embed.device)
        return self._bound().decode(img_seq)

    @torch.inference_mode()
    def infer(self, img):
        """decode(get_codebook_indices(img)) (dvae.py:354-358)"""
        self._require_decoder("infer")
        return self.decode(self.get_codebook_indices(img))

    @torch.inference_mode()
    def forward(self, img):
        """eval mode (dvae.py:363-381): img [B,channels,T] -> (recon_loss, commitment_loss, out [B,channels,T]), the losses 0-d"""
        if self.training:
            raise NotImplementedError("DiscreteVAE.forward: training mode is not supported (call .eval(): only the eval-mode "
                                      "branch, which decodes the quantised codes, is implemented)")
        self._require_decoder("forward")
        up = 2 ** self.cfg["num_layers"]
        if img.shape[-1] % up:
            raise ValueError(f"DiscreteVAE.forward: {img.shape[-1]} frames are not a multiple of {up} (the decoder returns "
                             f"{up} frames per code)")
        losses, out, _ = self._bound().reconstruct(img.to(torch.float32).contiguous())
        return losses[0], losses[1], out

    @torch.inference_mode()
    def get_codebook_indices(self, images):
        """images [B,channels,T] -> int64 [B,Tc]"""
        if self._engine is None:
            self.bind()
        images = images.to(torch.float32)
        if not images.is_contiguous() and images.transpose(1, 2).is_contiguous():
            # the harness passes `content_feat.transpose(1, 2)`: hand the frame-major storage over as it is
            return self._engine.encode(images.transpose(1, 2), frames_major=True).long()
        return self._engine.encode(images.contiguous()).long()
