"""Listen to the acoustic DVAE without the vocoder: wav -> 1024-point mel -> audio codes -> decoded mel -> inverse mel scale and
Griffin-Lim -> wav (GenVCModel.audition_codes; reference utils.py:164-172 is how the reference hears a DVAE).

    python scripts/audition_dvae.py --src_wav in.wav --output_path out.wav [--model_path ckpt.pth | --synthetic [--tiny]]
                                    [--n_iter 64] [--seed 0] [--save_codes codes.npy]

The waveform is peak-normalised only at the file writer (Griffin-Lim on a power spectrogram has no calibrated level); the tensor
`audition_codes` returns is untouched."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from genvc_amd import config as gcfg                                                   # noqa: E402
from genvc_amd.audio import load_audio, save_wav                                       # noqa: E402
from genvc_amd.inference.model_init import model_init, model_init_synthetic            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model_path", type=str, default="pre_trained/GenVC_large.pth")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--src_wav", type=str, required=True)
    ap.add_argument("--output_path", type=str, required=True)
    ap.add_argument("--synthetic", action="store_true", help="deterministic synthetic weights instead of --model_path")
    ap.add_argument("--tiny", action="store_true", help="with --synthetic: the small test architecture")
    ap.add_argument("--n_iter", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--save_codes", type=str, default=None, metavar="PATH.npy")
    args = ap.parse_args()
    if args.synthetic:
        model, _ = model_init_synthetic(gcfg.default_config(tiny=args.tiny, with_acoustic=True), seed=3, device=args.device)
    else:
        model, _ = model_init(args.model_path, args.device)
    if model.acoustic_dvae is None:
        raise SystemExit("audition_dvae: the checkpoint has no acoustic DVAE (acoustic_dvae_config and acoustic_dvae.* tensors)")
    sr = int(model.acoustic_sample_rate)
    wav = load_audio(args.src_wav, sr, device=args.device)
    if wav is None:
        raise SystemExit(f"audition_dvae: cannot read {args.src_wav}")
    mel = model.torch_mel_spectrogram_dvae(wav.to(args.device))
    up = 2 ** int(model.config.acoustic_dvae_config.num_layers)
    if mel.shape[-1] < up:
        raise SystemExit(f"audition_dvae: {wav.shape[-1]} samples give {mel.shape[-1]} mel frames, fewer than one code ({up} frames)")
    codes = model.acoustic_dvae.get_codebook_indices(mel)
    if args.save_codes:
        np.save(args.save_codes, codes.cpu().numpy())
    out = model.audition_codes(codes, n_iter=args.n_iter, seed=args.seed)
    peak = float(out.abs().max())
    if not np.isfinite(peak):
        raise SystemExit("audition_dvae: the inverted waveform is not finite (the decoded mel is out of range)")
    save_wav(args.output_path, out[0] * (0.95 / peak if peak > 0 else 1.0), sr)
    print(f"{args.output_path}: {codes.shape[1]} codes -> {out.shape[1]} samples at {sr} Hz ({args.n_iter} Griffin-Lim iterations, "
          f"seed {args.seed}, peak before normalisation {peak:.4g})")


if __name__ == "__main__":
    with torch.inference_mode():
        main()
