"""tests/golden/contrastive_search.npz: contrastive search (transformers 4.33's contrastive_search + _ranking_fast, the mode the reference's
`GPT.generate(top_k=K, do_sample=False, penalty_alpha=a)` selects under its pin, layers/gpt.py:594-609) driven on the reference's OWN
GPT2InferenceModel forward with output_hidden_states (layers/gpt_inference.py).  transformers 4.33 is not installed and the installed one
sends this mode to a Hub repository, so the loop is restated here around the reference forward: the prompt forward gives
ln_f of every prompt row (hidden_states[-1]) and the last logits; every step processes the logits (tests/proc_oracle.py), takes the
top-K of the softmax, runs the K candidates as one [B*K, 1] forward on the item's cache repeated K times (DynamicCache.
batch_repeat_interleave), ranks them and keeps the chosen candidate's cache rows (batch_select_indices).
Each case stores its inputs' seeds and settings, the ids, and the margin screens the tests re-assert; the CPU restatement on the
oracle's forward (tests/cs_oracle.py) must reproduce the ids, every case must differ from its greedy ids (alpha = 0), at least one
step must choose a candidate other than the most probable, and every processor kwarg a case sets must change its ids when it is dropped
(case d runs without the repetition penalty, with no_repeat_ngram_size=1 and a stop bias that puts eos among the candidates before
min_new_tokens is reached)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import make_golden as MG      # noqa: E402
from genvc_amd import config as gcfg      # noqa: E402
from genvc_amd import synth               # noqa: E402
import cs_oracle as CO                    # noqa: E402

PROB_GAP, SCORE_GAP = 1e-3, 1e-4


@torch.inference_mode()
def ref_contrastive(g, cond, codes, K, alpha, rep, max_new, kw):
    from transformers import DynamicCache
    gi = g.gpt_inference
    eos = g.stop_audio_token
    fake = g.compute_embeddings(cond, codes)
    B, n0 = fake.shape
    out = gi(input_ids=fake, past_key_values=DynamicCache(), attention_mask=torch.ones(B, n0, dtype=torch.long), use_cache=True,
             output_hidden_states=True, return_dict=True)
    ctx = out.hidden_states[-1]
    logits = out.logits[:, -1]
    cache = out.past_key_values
    cache.batch_repeat_interleave(K)
    rows = [list(map(int, r)) for r in fake]
    fin = [False] * B
    ar = torch.arange(B)
    toks = []
    for t in range(max_new):
        s = CO.process_rows(logits, rows, n0, rep, kw, eos)
        pk, tk = torch.topk(torch.softmax(s, -1), K, dim=-1)
        am = torch.ones(B * K, n0 + t + 1, dtype=torch.long)
        o = gi(input_ids=tk.reshape(-1, 1), past_key_values=cache, attention_mask=am, use_cache=True, output_hidden_states=True,
               return_dict=True)
        h = o.hidden_states[-1][:, -1].view(B, K, -1)
        sel, _ = CO.rank(ctx, h, pk, alpha)
        tok = [eos if fin[b] else int(tk[b, sel[b]]) for b in range(B)]
        for b in range(B):
            rows[b].append(tok[b])
            fin[b] = fin[b] or tok[b] == eos
        toks.append(tok)
        ctx = torch.cat([ctx, h[ar, sel].unsqueeze(1)], 1)
        logits = o.logits[:, -1].view(B, K, -1)[ar, sel]
        cache = o.past_key_values
        cache.batch_select_indices((ar * K + sel).repeat_interleave(K))
        if all(fin):
            break
    return np.array(toks, dtype=np.int64).T


def make_case(GPT, tag, model_args, seed, in_seeds, B, Tc, K, alphas, rep, max_new, kw=None, stop_bias=None, need_ragged=False):
    dims = gcfg.gpt_dims(model_args)
    w = synth.make_weights(seed, synth.gpt_weight_spec(dims))
    if stop_bias is not None:
        w["mel_head.bias"][1025] = float(stop_bias)
    g = MG.build_ref_gpt(GPT, model_args, w)
    for in_seed in in_seeds:
        cond, codes = MG.gpt_inputs(in_seed, dims, B, Tc)
        res, ok = [], True
        for a in alphas:
            r = CO.search(w, dims, cond, codes, K, a, rep, max_new, kw)
            greedy = CO.search(w, dims, cond, codes, K, 0.0, rep, max_new, kw)["ids"]
            why = None
            if r["prob_gap"] < PROB_GAP or r["score_gap"] < SCORE_GAP:
                why = f"gaps {r['prob_gap']:.1e} / {r['score_gap']:.1e}"
            elif not r["off_top1"] or (greedy.shape == r["ids"].shape and np.array_equal(greedy, r["ids"])):
                why = "no step leaves the top-1"
            elif need_ragged and len({int((row == 1025).argmax()) if (row == 1025).any() else -1 for row in r["ids"]}) < 2:
                why = "not ragged"
            else:
                for key in sorted(kw or {}):
                    rest = {k: v for k, v in kw.items() if k != key}
                    ids = CO.search(w, dims, cond, codes, K, a, rep, max_new, rest)["ids"]
                    if ids.shape == r["ids"].shape and np.array_equal(ids, r["ids"]):
                        why = f"{key} does not change the ids"
                        break
            if why is None:
                ids = ref_contrastive(g, cond, codes, K, a, rep, max_new, kw)
                if not np.array_equal(ids, r["ids"]):
                    why = "oracle differs from the reference forward"
            if why:
                print(f"  {tag}: in_seed {in_seed} alpha {a} rejected ({why})")
                ok = False
                break
            res.append((a, r))
        if ok:
            break
    else:
        raise RuntimeError(f"{tag}: no input seed passed the screen")
    out = {}
    for i, (a, r) in enumerate(res):
        p = f"{tag}_{i}_"
        out.update({p + "ids": r["ids"], p + "alpha": np.float64(a), p + "prob_gap": np.float64(r["prob_gap"]),
                    p + "score_gap": np.float64(r["score_gap"])})
    kw = kw or {}
    out.update({f"{tag}_seed": np.int64(seed), f"{tag}_in_seed": np.int64(in_seed), f"{tag}_B": np.int64(B), f"{tag}_Tc": np.int64(Tc),
                f"{tag}_K": np.int64(K), f"{tag}_n": np.int64(len(res)), f"{tag}_rep": np.float64(rep), f"{tag}_max_new": np.int64(max_new),
                f"{tag}_stop_bias": np.float64(stop_bias if stop_bias is not None else 0.0),
                f"{tag}_ngram": np.int64(kw.get("no_repeat_ngram_size", 0)), f"{tag}_min_new": np.int64(kw.get("min_new_tokens", 0)),
                f"{tag}_full": np.int64(model_args is gcfg.DEFAULT_MODEL_ARGS)})
    print(f"{tag}: in_seed {in_seed}, ids {[r['ids'].shape for _, r in res]}, gaps {min(r['prob_gap'] for _, r in res):.2e} / "
          f"{min(r['score_gap'] for _, r in res):.2e}")
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    GPT, _ = MG.import_reference()
    out = {}
    tiny = gcfg.TINY_MODEL_ARGS
    out.update(make_case(GPT, "a", tiny, 41, range(4100, 4160), B=1, Tc=9, K=2, alphas=[0.6], rep=2.0, max_new=24))
    out.update(make_case(GPT, "b", tiny, 43, range(4300, 4360), B=1, Tc=10, K=4, alphas=[0.6], rep=2.0, max_new=24))
    out.update(make_case(GPT, "c", tiny, 47, range(4700, 4800), B=3, Tc=11, K=2, alphas=[0.5], rep=2.0, max_new=32,
                         stop_bias=float(os.environ.get("CS_STOP_BIAS", "2.0")), need_ragged=True))
    out.update(make_case(GPT, "d", tiny, 53, range(5300, 5360), B=2, Tc=8, K=3, alphas=[0.4], rep=1.0, max_new=24,
                         kw=dict(no_repeat_ngram_size=1, min_new_tokens=10), stop_bias=2.0))
    if os.environ.get("CS_FULL", "1") == "1":
        out.update(make_case(GPT, "e", gcfg.DEFAULT_MODEL_ARGS, 3, range(500, 520), B=1, Tc=13, K=4, alphas=[0.3, 0.6], rep=10.0,
                             max_new=int(os.environ.get("CS_FULL_STEPS", "24"))))
    np.savez_compressed(os.path.join(MG.GOLD, "contrastive_search.npz"), **out)


if __name__ == "__main__":
    main()
