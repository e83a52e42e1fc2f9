"""Teacher-forced passes of the CPU oracle (oracle/genvc_oracle.py) over ONE slot's cache, for the tests of the primitives that continue
or rearrange an existing KV cache (tests/test_gpu_cache_ops_modes.py): a prefill, T forced tokens appended at a given mel position --
in one multi-row pass, as gvc_gpt_verify runs them, or token by token, as gvc_gpt_decode_step does -- and the rollback.

The rounding points of the storage modes are arguments, because a context picks them per call from the path the call takes:
  weights     `round_weights` (the matrices a bf16 context rounds at bind time) is applied by the caller, once;
  kv          dims["kv_bf16"]: k / v rounded as they enter the cache (weight_dtype >= 2);
  act         per call: the four activations of a block that cross a hand-off are rounded to bf16 (dims["act_bf16"]; the one-launch
              rows step of weight_dtype 3 and 4, every other multi-row pass of weight_dtype 4)."""
import torch

from oracle import genvc_oracle as O

BLOCK_MATRICES = ("attn.c_attn.weight", "attn.c_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


def round_weights(w):
    """the matrices a bf16-weights context rounds at bind time (include/genvc_hip.h: weight_dtype), in the weights' own dtype"""
    return {k: (O._bf16(v) if k.endswith(BLOCK_MATRICES) or k == "mel_head.weight" else v) for k, v in w.items()}


def prefill(w, dims, cond, codes, act=False):
    """[cond | <s> codes </s> | start] of one or more slots of equal length -> (latent, logits, cache) of the last row; the cache holds
    32 + Tc + 3 positions and the next forced token enters at mel position 1"""
    prefix = O.compute_embeddings(w, dims, cond, codes)[0]
    return O.gpt_prefill(w, dict(dims, act_bf16_prefill=bool(act)), prefix)


def forced_rows(w, dims, cache, toks, j0, act=False, stepwise=False):
    """toks: T forced tokens (1-D) of one slot whose cache holds `base` positions and whose next mel position is j0.
    -> (logits [T, V], latents [T, d], cache with base + T positions).  stepwise=False: one causal pass over the T rows (row t sees
    base + t + 1 keys); stepwise=True: T passes of one row.  The two are the same function of the inputs."""
    toks = torch.as_tensor(toks).long().view(-1)
    T = int(toks.numel())
    dm = dict(dims, act_bf16=bool(act))
    if stepwise:
        zs, ls = [], []
        for t in range(T):
            z, logits, cache = O.gpt_decode_step(w, dm, cache, toks[t:t + 1], j0 + t)
            zs.append(z[0])
            ls.append(logits[0])
        return torch.stack(ls), torch.stack(zs), cache
    emb = (w["mel_embedding.weight"][toks] + w["mel_pos_embedding.emb.weight"][j0:j0 + T]).unsqueeze(0)
    h, cache = O.gpt_blocks(w, dm, emb, cache)
    z, logits = O.head(w, h[0])
    return logits, z, cache


def rollback(cache, drop):
    """the cache without its last `drop` positions (gvc_gpt_truncate moves the length; the rows behind it are dead)"""
    if drop <= 0:
        return cache
    return [(k[:, :, :k.shape[2] - drop], v[:, :, :v.shape[2] - drop]) for k, v in cache]


def cache_len(cache):
    return int(cache[0][0].shape[2])
