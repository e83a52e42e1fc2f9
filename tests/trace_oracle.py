"""CPU restatement of the trace pass (include/genvc_hip.h: gvc_gpt_trace) on tests/forward_oracle.py's blocks: one teacher-forced pass
over [prefix | start, codes 0 .. n-2] that keeps every layer's attention weights and every hidden state, in float32 or, with float64
weights and inputs, in float64.  test_trace_host.py pins it against tests/golden/trace_*.npz (written by scripts/make_trace_golden.py
from the reference's GPT2InferenceModel driven step by step); the GPU tests use it where a fixture cannot reach (the device's own
sampled ids, other presets)."""
import numpy as np
import torch

from forward_oracle import CASES as _FWD_CASES, _gelu_new, _ln
from genvc_amd import config as gcfg
from genvc_amd import synth

import act_stats

# dims of the fixture cases: tests/forward_oracle.py's three (4 x 64, 4 x 256, 16 x 64) and a d 1024 case with 8 heads for HD 128
CASES = dict(_FWD_CASES, hd128=dict(gcfg.TINY_MODEL_ARGS, gpt_n_model_channels=1024, gpt_n_heads=8))
# per case: items, content codes, greedy steps (T = 32 + Tc + 2 + steps: no multiple of 16, past one 64-key chunk), the seed the
# screen starts from, and for `tiny` the stop-token bias search that ends one row early (oracle.make_golden.make_eos' habit)
SHAPES = {
    "tiny": dict(B=2, Tc=9, steps=24, seed=41, ragged=True),
    "hd256": dict(B=1, Tc=9, steps=24, seed=81, ragged=False),
    "hd64": dict(B=1, Tc=9, steps=24, seed=121, ragged=False),
    "hd128": dict(B=1, Tc=9, steps=24, seed=161, ragged=False),
}
PEAKED = dict(peaked=3.0)      # act_stats knob of the fixtures (a dict preset): score std ~3, a few keys carry a row
MIN_PEAK = 4.0                 # per layer: median over the stored rows of max_k p * (number of keys)
MIN_MARGIN = 2e-3              # the screen of oracle.make_golden.make_gpt
HIDDEN_STEP = 8                # wide cases keep every 8th channel of the hidden states
N_COND = 32


def case_dims(tag):
    return gcfg.gpt_dims(CASES[tag])


def case_weights(tag, seed, stop_bias=None, preset=PEAKED):
    """float32 weights of a case: synth weights of `seed` under the act_stats preset, the stop-token bias raised for the ragged case"""
    dims = case_dims(tag)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    w = act_stats.gpt_weights(w, dims, preset, seed=seed)
    if stop_bias is not None:
        w = dict(w)
        b = w["mel_head.bias"].clone()
        b[dims["stop_audio_token"]] = float(stop_bias)
        w["mel_head.bias"] = b
    return w


def case_inputs(tag, in_seed):
    dims, sh = case_dims(tag), SHAPES[tag]
    cond = synth.uniform(in_seed, "cond_latents", (sh["B"], N_COND, dims["d_model"]), 1.0)
    codes = synth.integers(in_seed, "content_codes", (sh["B"], sh["Tc"]), 256)
    return cond, codes


def lengths_of(tokens, stop):
    """generated length per row, the stop code counted; n for a row that never stopped.  tokens [B, n] (numpy or torch)"""
    t = torch.as_tensor(np.asarray(tokens))
    is_stop = t == stop
    first = is_stop.long().argmax(1) + 1
    return torch.where(is_stop.any(1), first, torch.full_like(first, t.shape[1]))


def trace(w, dims, cond, codes, tokens, lengths=None):
    """(probs [L,B,H,T,T], hidden [L+1,B,T,d]) of the pass over [cond | start text, codes, stop text | start audio, tokens[:, :n-1]],
    in the dtype of the weights.  Rows t >= P + lengths[b] are zeroed in both, as the device writes them (lengths None: nothing is)."""
    dt = w["gpt.ln_f.weight"].dtype
    B, n = tokens.shape
    text = torch.nn.functional.pad(torch.nn.functional.pad(codes, (0, 1), value=dims["stop_text_token"]), (1, 0),
                                   value=dims["start_text_token"])
    audio = torch.cat([torch.full((B, 1), dims["start_audio_token"], dtype=torch.long), tokens[:, :n - 1].long()], 1)
    temb = w["text_embedding.weight"][text] + w["text_pos_embedding.emb.weight"][:text.shape[1]]
    memb = w["mel_embedding.weight"][audio] + w["mel_pos_embedding.emb.weight"][:n]
    x = torch.cat([cond.to(dt), temb, memb], dim=1)
    _, T, d = x.shape
    P = T - n
    H, L = dims["n_head"], dims["n_layer"]
    hd = d // H
    causal = torch.arange(T).view(1, T) > torch.arange(T).view(T, 1)
    probs, hidden = [], [x]
    for l in range(L):
        p = f"gpt.h.{l}."
        qkv = _ln(x, w, p + "ln_1") @ w[p + "attn.c_attn.weight"] + w[p + "attn.c_attn.bias"]
        q, k, v = (t.reshape(B, T, H, hd).transpose(1, 2) for t in qkv.split(d, dim=-1))
        s = torch.matmul(q, k.transpose(-1, -2)) * hd ** -0.5
        pr = torch.softmax(s.masked_fill(causal, float("-inf")), dim=-1)
        probs.append(pr)
        o = torch.matmul(pr, v).transpose(1, 2).reshape(B, T, d)
        x = x + (o @ w[p + "attn.c_proj.weight"] + w[p + "attn.c_proj.bias"])
        h = _gelu_new(_ln(x, w, p + "ln_2") @ w[p + "mlp.c_fc.weight"] + w[p + "mlp.c_fc.bias"])
        x = x + (h @ w[p + "mlp.c_proj.weight"] + w[p + "mlp.c_proj.bias"])
        hidden.append(x if l < L - 1 else _ln(x, w, "gpt.ln_f"))
    probs, hidden = torch.stack(probs), torch.stack(hidden)
    if lengths is not None:
        dead = torch.arange(T).view(1, T) >= (P + torch.as_tensor(lengths).view(B, 1))          # [B, T]
        probs = probs.masked_fill(dead[None, :, None, :, None], 0.0)
        hidden = hidden.masked_fill(dead[None, :, :, None], 0.0)
    return probs, hidden


def alignment(probs, P, n, n_cond, Tc, layers=None):
    """mean over the heads of the chosen layers of the step rows' weight on the content key rows: [B, n, Tc] in float64"""
    pr = probs.double()
    if layers is not None:
        pr = pr[[l % pr.shape[0] for l in layers]]
    return pr[:, :, :, P:P + n, n_cond + 1:n_cond + 1 + Tc].mean(dim=(0, 2))


def steps_of(probs, hidden, P, n):
    """the full tensors cut into HF's per-step structure: (attentions, hidden_states), each a tuple over the n steps of tuples over
    the layers.  Step 0: [B,H,P+1,P+1] / [B,P+1,d]; step i: [B,H,1,P+1+i] / [B,1,d]"""
    att, hid = [], []
    for i in range(n):
        lo = 0 if i == 0 else P + i
        att.append(tuple(probs[l][:, :, lo:P + i + 1, :P + i + 1] for l in range(probs.shape[0])))
        hid.append(tuple(hidden[l][:, lo:P + i + 1] for l in range(hidden.shape[0])))
    return tuple(att), tuple(hid)


def peak(probs_rows, n_keys):
    """max_k p * (number of keys) of rows [..., keys] with n_keys live keys each ([...] int tensor or int)"""
    return probs_rows.amax(-1) * n_keys


def stored_peak_median(att_steps, lengths):
    """per layer: the median over the live stored rows (all heads, all items) of max_k p * keys.  att_steps: HF's structure"""
    L = len(att_steps[0])
    out = []
    for l in range(L):
        vals = []
        for i, step in enumerate(att_steps):
            a = torch.as_tensor(np.asarray(step[l])).double()            # [B,H,rows,keys]
            keys = a.shape[-1]
            first = keys - a.shape[-2]
            nk = torch.arange(first + 1, keys + 1).view(1, 1, -1).double()
            live = (torch.as_tensor(lengths).view(-1, 1, 1) > i).expand(a.shape[0], a.shape[1], a.shape[2])
            vals.append((a.amax(-1) * nk)[live])
        out.append(float(torch.cat(vals).median()))
    return out
