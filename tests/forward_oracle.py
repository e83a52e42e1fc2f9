"""CPU restatement of the evaluation pass of GPT.forward (reference layers/gpt.py:375-537) on a weight dict, in plain torch: the masked
Perceiver, the block stack with a key-padding mask, both heads, the losses and the top-10 hit count.  test_forward_eval_host.py pins it
against tests/golden/forward_eval_*.npz (written by scripts/make_forward_golden.py from the reference's own classes); the GPU tests use
it where a fixture cannot reach (perturbed inputs, single items)."""
import math

import torch
import torch.nn.functional as F

from genvc_amd import config as gcfg
from genvc_amd import synth

CASES = {
    "tiny": gcfg.TINY_MODEL_ARGS,
    "hd256": dict(gcfg.TINY_MODEL_ARGS, gpt_n_model_channels=1024, gpt_n_heads=4),
    "hd64": dict(gcfg.TINY_MODEL_ARGS, gpt_n_model_channels=1024, gpt_n_heads=16),
}
COND_FRAMES = 300
MIN_MARGIN = 2e-3          # the screen of scripts/make_forward_golden.py


def load(gold, tag):
    """a case's fixture as a dict, the tiny case's full mel_logits put together again"""
    g = dict(gold(f"forward_eval_{tag}"))
    if tag == "tiny":
        import numpy as np
        g["mel_logits"] = np.concatenate([gold("forward_eval_tiny_logits0")["mel_logits_items01"],
                                          gold("forward_eval_tiny_logits1")["mel_logits_item2"]])
    return g


def inputs(g, dims):
    """what the fixture script derives from the seed: text ids, conditioning latents, conditioning mels; and the stored codes / lengths"""
    seed, B = int(g["seed"]), len(g["text_lengths"])
    text = synth.integers(seed, "fe_text", (B, int(g["text_lengths"].max()) + 3), 256)
    cond = synth.uniform(seed, "cond_latents", (B, 32, dims["d_model"]), 1.0)
    mels = synth.uniform(seed, "fe_cond_mels", (B, 80, COND_FRAMES), 1.0)
    t = lambda k: torch.from_numpy(g[k])
    return dict(text=text, cond=cond, mels=mels, codes=t("codes"), text_lengths=t("text_lengths"), wav_lengths=t("wav_lengths"),
                cond_lens=t("cond_lens"))


def _ln(x, w, name):
    return F.layer_norm(x, (x.shape[-1],), w[name + ".weight"], w[name + ".bias"], 1e-5)


def _gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def perceiver(w, x, mask=None, prefix="conditioning_perceiver.", heads=8, dim_head=64):
    """PerceiverResampler.forward(x [B,F,80], mask bool [B, F + 32]): mask entry j meets key j of cat([latents, frames])"""
    g = lambda n: w[prefix + n]
    B = x.shape[0]
    x = F.linear(x, g("proj_context.weight"), g("proj_context.bias"))
    lat = g("latents").unsqueeze(0).expand(B, -1, -1)
    l = 0
    while f"{prefix}layers.{l}.0.to_q.weight" in w:
        p = f"layers.{l}."
        ctx = torch.cat((lat, x), dim=-2)
        q = F.linear(lat, g(p + "0.to_q.weight"))
        k, v = F.linear(ctx, g(p + "0.to_kv.weight")).chunk(2, dim=-1)
        sh = lambda t: t.reshape(B, t.shape[1], heads, dim_head).transpose(1, 2)
        sim = torch.matmul(sh(q), sh(k).transpose(-1, -2)) * dim_head ** -0.5
        if mask is not None:
            sim = sim.masked_fill(~mask[:, None, None, :], -torch.finfo(sim.dtype).max)
        o = torch.matmul(sim.softmax(dim=-1), sh(v)).transpose(1, 2).reshape(B, lat.shape[1], heads * dim_head)
        lat = F.linear(o, g(p + "0.to_out.weight")) + lat
        a, gate = F.linear(lat, g(p + "1.0.weight"), g(p + "1.0.bias")).chunk(2, dim=-1)
        lat = F.linear(F.gelu(gate) * a, g(p + "1.2.weight"), g(p + "1.2.bias")) + lat
        l += 1
    return F.normalize(lat, dim=-1) * lat.shape[-1] ** 0.5 * g("norm.gamma")


def blocks(w, dims, x, key_mask=None):
    """the GPT-2 block stack on rows x [B,T,d]: causal attention, keys with key_mask [B,T] == False left out for every query row"""
    B, T, d = x.shape
    H = dims["n_head"]
    hd = d // H
    causal = torch.arange(T).view(1, T) > torch.arange(T).view(T, 1)
    for l in range(dims["n_layer"]):
        p = f"gpt.h.{l}."
        qkv = _ln(x, w, p + "ln_1") @ w[p + "attn.c_attn.weight"] + w[p + "attn.c_attn.bias"]
        q, k, v = (t.reshape(B, T, H, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        s = torch.matmul(q, k.transpose(-1, -2)) * hd ** -0.5
        s = s.masked_fill(causal, float("-inf"))
        if key_mask is not None:
            s = s.masked_fill(~key_mask[:, None, None, :], float("-inf"))
        o = torch.matmul(torch.softmax(s, dim=-1), v).transpose(1, 2).reshape(B, T, d)
        x = x + (o @ w[p + "attn.c_proj.weight"] + w[p + "attn.c_proj.bias"])
        h = _gelu_new(_ln(x, w, p + "ln_2") @ w[p + "mlp.c_fc.weight"] + w[p + "mlp.c_fc.bias"])
        x = x + (h @ w[p + "mlp.c_proj.weight"] + w[p + "mlp.c_proj.bias"])
    return _ln(x, w, "gpt.ln_f")


def latents(w, dims, cond, text_ids, code_ids, key_mask=None):
    """final_norm(ln_f(h)) of the text and code rows [B, Lt + Lm, d]"""
    temb = w["text_embedding.weight"][text_ids] + w["text_pos_embedding.emb.weight"][:text_ids.shape[1]]
    memb = w["mel_embedding.weight"][code_ids] + w["mel_pos_embedding.emb.weight"][:code_ids.shape[1]]
    h = blocks(w, dims, torch.cat([cond, temb, memb], dim=1), key_mask)
    return _ln(h[:, cond.shape[1]:], w, "final_norm")


def loss_and_hits(logits, targets, label_smoothing=0.0, top_k=10):
    """the reduction the device runs (csrc/forward_eval.hip), restated: logits [R,V], targets [R] with -1 ignored -> (loss, hits, count).
    nll = lse - x[t]; smoothing term = lse - mean x; hit = #{x > x[t]} < top_k; loss = ((1 - ls) sum nll + ls sum smoothing) / count"""
    keep = targets >= 0
    x, t = logits[keep].double(), targets[keep]
    lse = torch.logsumexp(x, dim=1)
    xt = x.gather(1, t[:, None])[:, 0]
    nll, smooth = lse - xt, lse - x.mean(dim=1)
    hits = int(((x > xt[:, None]).sum(1) < top_k).sum())
    n = int(keep.sum())
    return float(((1 - label_smoothing) * nll.sum() + label_smoothing * smooth.sum()) / n), hits, n


def forward(w, dims, prep, cond, label_smoothing=0.0):
    """the default call from prepared ids: (loss_text, loss_mel, hits, count, mel_logits [B,V,Lm])"""
    Lt = prep["text_ids"].shape[1]
    lat = latents(w, dims, cond, prep["text_ids"], prep["code_ids"], prep["key_mask"])
    tl = F.linear(lat[:, :Lt], w["text_head.weight"], w["text_head.bias"])
    ml = F.linear(lat[:, Lt:], w["mel_head.weight"], w["mel_head.bias"])
    lt, _, _ = loss_and_hits(tl.reshape(-1, tl.shape[-1]), prep["text_targets"].reshape(-1), label_smoothing)
    lm, hits, n = loss_and_hits(ml.reshape(-1, ml.shape[-1]), prep["mel_targets"].reshape(-1), label_smoothing)
    return lt, lm, hits, n, ml.permute(0, 2, 1)
