"""Generate tests/golden/forward_eval_*.npz: the reference's GPT.forward evaluation pass (layers/gpt.py:375-537) on synthetic weights.

Runs only where the reference checkout is present (oracle.make_golden.import_reference); nothing of it is copied -- its classes are
imported, loaded with genvc_amd.synth weights and called, and hooks record what they were given.

    python scripts/make_forward_golden.py [--only tiny|hd256|hd64]

Per case (a ragged batch of 3: text lengths 40 / 5 / 23, 12 / 3 / 20 codes, 300 / 40 / 20 conditioning frames) one file with
  * the inputs that are not re-derived from the seed (the designed codes, the lengths);
  * the prepared ids, targets and masks, captured by hooks on the embeddings, on get_logits, on the Perceiver and on F.cross_entropy;
  * the four outputs of the GPT-only call (cond_latents given) at label_smoothing 0 and 0.1, and of the end-to-end call
    (cond_mels + cond_lens); the masked get_style_emb output; the ragged return_latent=True output;
  * the top-10 hit count by the published definition of torchmetrics MulticlassAccuracy(top_k=10, average="micro", ignore_index=-1)
    (torchmetrics is stubbed here): the share of non-ignored positions whose target is among the 10 largest logits.
The codes are built position by position from the reference's own logits so that the targets have designed ranks (cycling 1, 3, 9,
10, 11, 12, 400): the accuracy is neither 0 nor 1.  Seeds are screened as make_gpt screens them: a fixture is kept only if every valid
position's target logit is at least 2e-3 away from the boundary between the 10th and the 11th largest logit.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
from oracle.make_golden import GOLD, build_ref_gpt, import_reference      # noqa: E402

CASES = {
    "tiny": gcfg.TINY_MODEL_ARGS,                                                               # d 256, 4 heads x 64
    "hd256": dict(gcfg.TINY_MODEL_ARGS, gpt_n_model_channels=1024, gpt_n_heads=4),              # d 1024, 4 heads x 256
    "hd64": dict(gcfg.TINY_MODEL_ARGS, gpt_n_model_channels=1024, gpt_n_heads=16),              # d 1024, 16 heads x 64
}
TEXT_LENGTHS = [40, 5, 23]
N_CODES = [12, 3, 20]
WAV_LENGTHS = [12 * 1024 - 100, 3 * 1024 - 1000, 20 * 1024 - 511]          # no multiples of 1024
COND_FRAMES = [300, 40, 20]
COND_LENS = [300 * 256 + 17, 40 * 256 + 100, 20 * 256 + 255]               # samples, no multiples of 256
RANKS = [1, 3, 9, 10, 11, 12, 400]
MIN_MARGIN = 2e-3
VOCAB_STEP = 9                 # wide cases keep every 9th vocabulary entry of mel_logits (plus the start / stop tokens)


def inputs(seed, d):
    """everything the tests re-derive from the seed"""
    B = len(TEXT_LENGTHS)
    text = synth.integers(seed, "fe_text", (B, max(TEXT_LENGTHS) + 3), 256)
    cond = synth.uniform(seed, "cond_latents", (B, 32, d), 1.0)
    mels = synth.uniform(seed, "fe_cond_mels", (B, 80, max(COND_FRAMES)), 1.0)
    return text, cond, mels


def rank_stats(mel_logits, mel_targets):
    """hits, count and the screen margin over the valid positions.  mel_logits [B,V,L], targets [B,L] with -1 ignored"""
    x = mel_logits.permute(0, 2, 1).reshape(-1, mel_logits.shape[1]).double()
    t = mel_targets.reshape(-1)
    keep = t >= 0
    x, t = x[keep], t[keep]
    xt = x.gather(1, t[:, None])[:, 0]
    rank = (x > xt[:, None]).sum(1)
    top = x.topk(11, dim=1)[0]
    hit = rank < 10
    margin = torch.where(hit, xt - top[:, 10], top[:, 9] - xt)
    return int(hit.sum()), int(keep.sum()), float(margin.min()), rank


class Top10Accuracy(torch.nn.Module):
    """what the stubbed torchmetrics metric returns, by its published definition"""

    def forward(self, mel_logits, mel_targets):
        hits, count, _, _ = rank_stats(mel_logits, mel_targets)
        return torch.tensor(hits / count, dtype=torch.float32)


class Tap:
    """records what the reference hands to its embeddings, get_logits, the Perceiver and F.cross_entropy during one call"""

    def __init__(self, g, gpt_mod):
        self.g, self.mod, self.rec = g, gpt_mod, {}

    def __enter__(self):
        g, rec = self.g, self.rec
        self.h = [g.text_embedding.register_forward_pre_hook(lambda m, a: rec.__setitem__("text_ids", a[0].clone())),
                  g.mel_embedding.register_forward_pre_hook(lambda m, a: rec.__setitem__("code_ids", a[0].clone())),
                  g.conditioning_perceiver.register_forward_pre_hook(
                      lambda m, a, k: rec.__setitem__("perceiver_mask", None if k.get("mask") is None else k["mask"].clone()),
                      with_kwargs=True)]
        self.get_logits = g.get_logits

        def get_logits(*a, **k):
            for n in ("attn_mask_text", "attn_mask_mel"):
                if k.get(n) is not None:
                    rec[n] = k[n].clone()
            rec["n_cond"] = int(k["prompt"].shape[1])
            return self.get_logits(*a, **k)
        g.get_logits = get_logits
        self.ce = self.mod.F.cross_entropy
        rec["targets"] = []

        def cross_entropy(logits, targets, **k):
            rec["targets"].append((targets.clone(), dict(k)))
            return self.ce(logits, targets, **k)
        self.mod.F.cross_entropy = cross_entropy
        return rec

    def __exit__(self, *e):
        for h in self.h:
            h.remove()
        self.g.get_logits = self.get_logits
        self.mod.F.cross_entropy = self.ce


@torch.inference_mode()
def design_codes(g, text, tl, wl, cond):
    """codes whose targets have the designed ranks under the reference's own logits, position by position (causal: the logits of
    position i depend on the codes in front of it only)"""
    B, n_max = len(N_CODES), max(N_CODES)
    codes = torch.zeros(B, n_max, dtype=torch.long)
    dummy = torch.zeros(B, 1, 80, 4)
    for i in range(n_max):
        _, _, _, ml = g(text, tl, codes.clone(), wl, cond_mels=dummy, cond_latents=cond)
        order = ml[:, :, i].argsort(dim=1, descending=True)
        for b in range(B):
            if i >= N_CODES[b]:
                continue
            r = RANKS[(i + 2 * b) % len(RANKS)] - 1
            while int(order[b, r]) >= 1024:          # a code, not the start / stop token
                r += 1
            codes[b, i] = order[b, r]
    return codes


@torch.inference_mode()
def make_case(GPT, gpt_mod, tag, model_args, seed0):
    dims = gcfg.gpt_dims(model_args)
    d = dims["d_model"]
    tl, wl = torch.tensor(TEXT_LENGTHS), torch.tensor(WAV_LENGTHS)
    cl = torch.tensor(COND_LENS)
    dummy = torch.zeros(len(TEXT_LENGTHS), 1, 80, 4)
    for seed in range(seed0, seed0 + 20):
        w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
        g = build_ref_gpt(GPT, model_args, w)
        g.accuracy_metric = Top10Accuracy()
        text, cond, mels = inputs(seed, d)
        codes = design_codes(g, text, tl, wl, cond)
        with Tap(g, gpt_mod) as rec:
            lt0, lm0, _, ml = g(text, tl, codes.clone(), wl, cond_mels=dummy, cond_latents=cond)
        (tt, _), (mt, _) = rec["targets"]
        hits, count, margin, rank = rank_stats(ml, mt)
        if margin >= MIN_MARGIN:
            break
        print(f"  forward_eval_{tag}: seed {seed} rejected (margin {margin:.2e}, {hits} hits of {count})")
    else:
        raise RuntimeError("no seed passed the rank-margin screen")
    out = dict(seed=seed, text_lengths=tl.numpy(), wav_lengths=wl.numpy(), cond_lens=cl.numpy(), codes=codes.numpy(),
               text_ids=rec["text_ids"].numpy(), code_ids=rec["code_ids"].numpy(), text_targets=tt.numpy(), mel_targets=mt.numpy(),
               attn_mask_text=rec["attn_mask_text"].numpy(), attn_mask_mel=rec["attn_mask_mel"].numpy(), n_cond=rec["n_cond"],
               hits=hits, count=count, margin=margin, ranks=rank.numpy(), loss_text_ls0=float(lt0), loss_mel_ls0=float(lm0))
    g.label_smoothing = 0.1
    lt1, lm1, _, ml1 = g(text, tl, codes.clone(), wl, cond_mels=dummy, cond_latents=cond)
    assert torch.equal(ml, ml1)
    out.update(loss_text_ls1=float(lt1), loss_mel_ls1=float(lm1))
    g.label_smoothing = 0.0
    # the end-to-end call: cond_mels + cond_lens through the masked Perceiver
    with Tap(g, gpt_mod) as rec:
        e_lt, e_lm, _, e_ml = g(text, tl, codes.clone(), wl, cond_mels=mels.unsqueeze(1), cond_lens=cl)
    e_hits, e_count, e_margin, _ = rank_stats(e_ml, rec["targets"][1][0])
    style = g.get_style_emb(mels, seq_lens=cl // 256)                                   # [B, d, 32]
    relat = g(text, tl, codes.clone(), wl, cond_latents=cond, return_latent=True)       # [B, Lm - 5, d]
    out.update(perceiver_mask=rec["perceiver_mask"].numpy(), e2e_loss_text=float(e_lt), e2e_loss_mel=float(e_lm), e2e_hits=e_hits,
               e2e_count=e_count, e2e_margin=e_margin)
    V = ml.shape[1]
    ids = np.unique(np.concatenate([np.arange(0, V, VOCAB_STEP), [1024, 1025]]))
    out.update(vocab_ids=ids, mel_logits_sub=ml.numpy()[:, ids], e2e_mel_logits_sub=e_ml.numpy()[:, ids])
    if d <= 256:
        out.update(style=style.numpy(), relatents=relat.numpy())
        logits = [dict(mel_logits_items01=ml.numpy()[:2]), dict(mel_logits_item2=ml.numpy()[2:])]
    else:
        out.update(style=style.numpy()[:, ::8], relatents=relat.numpy()[:, :, ::8])
        logits = None
    path = os.path.join(GOLD, f"forward_eval_{tag}.npz")
    np.savez_compressed(path, **out)
    sizes = [os.path.getsize(path)]
    for i, part in enumerate(logits or []):       # the tiny case keeps every vocabulary entry of mel_logits, in two files of their own
        lp = os.path.join(GOLD, f"forward_eval_{tag}_logits{i}.npz")
        np.savez_compressed(lp, **part)
        sizes.append(os.path.getsize(lp))
    assert max(sizes) < 300 * 1024, sizes
    print(f"forward_eval_{tag}: seed {seed}, {hits} hits of {count} (margin {margin:.2e}); end to end {e_hits} of {e_count} "
          f"(margin {e_margin:.2e}); losses {float(lt0):.5f} {float(lm0):.5f} / {float(lt1):.5f} {float(lm1):.5f}; bytes {sizes}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    GPT, _ = import_reference()
    import layers.gpt as gpt_mod
    for i, (tag, model_args) in enumerate(CASES.items()):
        if args.only in (None, tag):
            make_case(GPT, gpt_mod, tag, model_args, 31 + 40 * i)


if __name__ == "__main__":
    main()
