"""Detect the green-list watermark in the per-segment codes that `infer.py --token_scores PATH.npz` writes.

    python scripts/detect_watermark.py --tokens scores.npz --watermark_key K [--watermark_ratio 0.25] [--watermark_scheme lefthash]
                                       [--z_threshold 3.0] [--ignore_repeated_ngrams]

Prints one line per segment and one for the whole utterance (the counts of the segments added up: under lefthash the first code of a
segment is never scored, its previous id being the prompt's).  The key is the secret: another key finds nothing.  The counts run on
the GPU (genvc_amd.engine.WatermarkDetector); z and p are transformers' formulas in float64."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tokens", required=True, metavar="PATH.npz", help="what infer.py --token_scores wrote (n_segments, tokens_i)")
    ap.add_argument("--watermark_key", type=int, required=True, metavar="K")
    ap.add_argument("--watermark_ratio", type=float, default=0.25, metavar="G")
    ap.add_argument("--watermark_scheme", type=str, default="lefthash", choices=("lefthash", "selfhash"))
    ap.add_argument("--vocab", type=int, default=1026, help="the code vocabulary of the model that generated the codes")
    ap.add_argument("--z_threshold", type=float, default=3.0)
    ap.add_argument("--ignore_repeated_ngrams", action="store_true")
    args = ap.parse_args(argv)
    import torch
    from genvc_amd.engine import WatermarkDetector, watermark_statistics
    cfg = dict(greenlist_ratio=args.watermark_ratio, hashing_key=args.watermark_key, seeding_scheme=args.watermark_scheme)
    try:
        det = WatermarkDetector(cfg, args.vocab, ignore_repeated_ngrams=args.ignore_repeated_ngrams)
    except (ValueError, NotImplementedError) as e:
        raise SystemExit(f"detect_watermark: {e}")
    z = np.load(args.tokens)
    n_seg = int(z["n_segments"])
    total = np.zeros((1, 2), dtype=np.int64)
    for i in range(n_seg):
        toks = np.asarray(z[f"tokens_{i}"]).reshape(-1)
        if toks.size == 0:
            print(f"segment {i}: no codes")
            continue
        counts, _ = det.counts(torch.from_numpy(toks.astype(np.int64)))
        c = counts.cpu().numpy().astype(np.int64)
        total += c
        s = watermark_statistics(c, args.watermark_ratio, args.z_threshold)
        print(f"segment {i}: {toks.size} codes, {int(c[0, 0])} scored, {int(c[0, 1])} green, z = {s['z_score'][0]:.3f}, "
              f"p = {s['p_value'][0]:.3g}, watermarked: {bool(s['prediction'][0])}")
    s = watermark_statistics(total, args.watermark_ratio, args.z_threshold)
    print(f"utterance: {n_seg} segments, {int(total[0, 0])} scored, {int(total[0, 1])} green, z = {s['z_score'][0]:.3f}, "
          f"p = {s['p_value'][0]:.3g}, watermarked: {bool(s['prediction'][0])}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
