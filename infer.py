"""CLI of the reference (/root/reference/infer.py:8-36) on the MI355X-native path.

Flags and defaults are the reference's; added: --seg_len (the reference hard-codes 6.0; the README's
"1-second chunk" numbers correspond to --seg_len 1.0), --stream_chunk_size, --synthetic (no checkpoint
ships with the reference: run the same pipeline on deterministic synthetic weights), --save_tokens, --token_scores and
--decode_codes_to_mel (the acoustic DVAE's mel of the generated codes).
The waveform is written like the reference does (24 kHz PCM16); --save_tokens also stores the codec tokens/latents.
"""
import argparse
import os

import torch

from genvc_amd.audio import load_audio, save_wav
from genvc_amd.inference.inference_utils import synthesize_utt, synthesize_utt_streaming
from genvc_amd.inference.model_init import model_init, model_init_synthetic

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--model_path", type=str, default="pre_trained/GenVC_large.pth")
    parser.add_argument("--device", type=str, default="cuda")
    parser.add_argument("--src_wav", type=str, default="samples/EF4_ENG_0112_1.wav")
    parser.add_argument("--ref_audio", type=str, default="samples/EM1_ENG_0037_1.wav")
    parser.add_argument("--output_path", type=str, default="samples/converted.wav")
    parser.add_argument("--top_k", type=int, default=15)
    parser.add_argument("--streaming", action="store_true")
    parser.add_argument("--seg_len", type=float, default=6.0)
    parser.add_argument("--stream_chunk_size", type=int, default=8)
    parser.add_argument("--synthetic", action="store_true", help="deterministic synthetic weights instead of --model_path")
    parser.add_argument("--tiny", action="store_true", help="with --synthetic: the 2-layer test architecture")
    parser.add_argument("--vocoder_resblock_type", type=str, default="2", choices=["1", "2"],
                        help="with --synthetic: the vocoder's residual block (1: ResBlock1 with the HiFi-GAN V1 kernels 3 / 7 / 11 and "
                             "dilations 1 / 3 / 5; a checkpoint brings its own vocoder_config.resblock_type)")
    parser.add_argument("--save_tokens", type=str, default=None)
    parser.add_argument("--weights", type=str, default="fp32", choices=["fp32", "bf16", "bf16_kv", "bf16_act", "bf16_mfma"],
                        help="GPT weight / KV-cache storage on the GPU (fp32 = the reference's numerics)")
    parser.add_argument("--num_beams", type=int, default=1,
                        help="non-streaming only: > 1 decodes with deterministic beam search (do_sample=False) of this width")
    parser.add_argument("--num_beam_groups", type=int, default=1,
                        help="with --num_beams K: > 1 splits the beams into this many groups (K a multiple of it) searched one after the "
                             "other, each penalised for the tokens the earlier groups chose (group beam search); needs --diversity_penalty")
    parser.add_argument("--diversity_penalty", type=float, default=None,
                        help="with --num_beam_groups > 1: the penalty (> 0) per earlier group's choice of the same token at a step")
    parser.add_argument("--penalty_alpha", type=float, default=None,
                        help="non-streaming only: > 0 decodes with contrastive search (do_sample=False) over --top_k candidates (2..16)")
    parser.add_argument("--num_return_sequences", type=int, default=1,
                        help="non-streaming only: N > 1 draws N candidates per segment from one prefill (or keeps the N best beams with "
                             "--num_beams >= N) and writes <output stem>_<j>.wav, printing one score per file")
    parser.add_argument("--min_new_tokens", type=int, default=None, help="no stop token before this many tokens per segment")
    parser.add_argument("--no_repeat_ngram_size", type=int, default=None,
                        help="no n-gram of codec tokens (fake prompt included) occurs twice in a segment (1..8)")
    parser.add_argument("--eos_decay", type=float, nargs=2, default=None, metavar=("START", "FACTOR"),
                        help="exponential_decay_length_penalty: from START new tokens on, the stop score grows by FACTOR per token")
    parser.add_argument("--min_p", type=float, default=None, help="min-p sampling cut-off in [0, 1]")
    parser.add_argument("--typical_p", type=float, default=None, help="typical sampling mass in (0, 1] (1: off)")
    parser.add_argument("--epsilon_cutoff", type=float, default=None, help="epsilon sampling cut-off in [0, 1) (0: off)")
    parser.add_argument("--eta_cutoff", type=float, default=None, help="eta sampling cut-off in [0, 1) (0: off)")
    parser.add_argument("--ras_window", type=int, default=None, metavar="K",
                        help="repetition-aware sampling: a token that fills its share of the last K generated codes (1..64) is drawn again "
                             "from the untruncated distribution; with --top_k 1 this is greedy decoding with an escape from loops")
    parser.add_argument("--ras_threshold", type=float, default=None, metavar="T",
                        help="with --ras_window: the share of the window in (0, 1] at which a token is drawn again (default 0.1)")
    parser.add_argument("--presence_penalty", type=float, default=None, metavar="X",
                        help="subtract X (in [-2, 2]) from the score of every code that occurs among the counted generated codes")
    parser.add_argument("--frequency_penalty", type=float, default=None, metavar="Y",
                        help="subtract Y (in [-2, 2]) times its count from the score of every code among the counted generated codes")
    parser.add_argument("--penalty_window", type=int, default=None, metavar="W",
                        help="count only the last W generated codes for --presence_penalty / --frequency_penalty, and apply "
                             "--repetition_penalty to those codes only (default: every generated code; the repetition penalty unchanged)")
    parser.add_argument("--watermark_key", type=int, default=None, metavar="K",
                        help="mark the generated codes with the green-list watermark under the hashing key K (an integer in [0, 2**63)); "
                             "scripts/detect_watermark.py --tokens PATH.npz --watermark_key K finds it in the codes --token_scores "
                             "writes.  With --top_k 1 pass --greedy: a marked greedy stream is greedy search (do_sample=False)")
    parser.add_argument("--watermark_bias", type=float, default=2.0, metavar="D", help="with --watermark_key: added to the green scores")
    parser.add_argument("--watermark_ratio", type=float, default=0.25, metavar="G",
                        help="with --watermark_key: the share of the codes that is green at a step, in (0, 1)")
    parser.add_argument("--watermark_scheme", type=str, default="lefthash", choices=("lefthash", "selfhash"),
                        help="with --watermark_key: transformers' seeding scheme")
    parser.add_argument("--greedy", action="store_true", help="greedy search (do_sample=False) instead of sampling")
    parser.add_argument("--sequence_bias", action="append", default=None, metavar="IDS=VALUE",
                        help="non-streaming only, repeatable: add VALUE to the score of the last of the comma-separated codec ids when the "
                             "ids before it were just generated (HF sequence_bias), e.g. 1025=-2.0 makes every segment stop later")
    parser.add_argument("--bad_words_ids", action="append", default=None, metavar="IDS",
                        help="non-streaming only, repeatable: never generate this comma-separated id sequence (HF bad_words_ids)")
    parser.add_argument("--forced_eos", action="store_true",
                        help="non-streaming only: a segment that reaches its token budget ends with the stop code (HF forced_eos_token_id)")
    parser.add_argument("--guidance_scale", type=float, default=None,
                        help="non-streaming only: classifier-free guidance strength (HF guidance_scale; 1 or absent: off): every segment "
                             "decodes under the reference speaker and under a negative speaker and extrapolates away from the negative")
    parser.add_argument("--negative_ref_audio", type=str, default=None,
                        help="with --guidance_scale: the negative speaker's audio (default: the source utterance, whose timbre leaks)")
    parser.add_argument("--token_scores", type=str, default=None, metavar="PATH.npz",
                        help="non-streaming only: write, per segment, the codec tokens and the log-probability of each under the "
                             "distribution it was decoded from (processors, warpers and guidance included)")
    parser.add_argument("--alignment", type=str, default=None, metavar="PATH.npz",
                        help="non-streaming only: write, per segment, the attention of every generated acoustic code over the segment's "
                             "content codes (head / layer mean, GPT.trace), its argmax content position and its attention mass on content")
    parser.add_argument("--assistant_layers", type=int, default=None, metavar="N",
                        help="with --synthetic, non-streaming: assisted (speculative) greedy decoding with a synthetic N-layer draft model "
                             "of the same width (GPT.generate(assistant_model=...)); a demonstration of the mode, not of an acceptance rate")
    parser.add_argument("--num_assistant_tokens", type=int, default=None, metavar="K",
                        help="with --assistant_layers: tokens drafted per round, 1..15 (default 5)")
    parser.add_argument("--assistant_sampling", action="store_true",
                        help="with --assistant_layers or --prompt_lookup_num_tokens: speculative sampling (GPT.generate(speculative_sampling=True)) -- the draft samples "
                             "and the sampling flags (--top_k, config top_p / temperature) apply; without it --assistant_layers decodes "
                             "greedily")
    parser.add_argument("--prompt_lookup_num_tokens", type=int, default=None, metavar="K",
                        help="non-streaming: prompt-lookup assisted decoding (GPT.generate(prompt_lookup_num_tokens=K)), K in 1..15 -- "
                             "every round drafts the K codes that followed the earliest earlier occurrence of the segment's last codes; "
                             "no draft model, so it runs on a real checkpoint; greedy, or sampled with --assistant_sampling")
    parser.add_argument("--max_matching_ngram_size", type=int, default=None, metavar="N",
                        help="with --prompt_lookup_num_tokens: the longest run of last codes searched for, 1..8 (default 2)")
    parser.add_argument("--decode_codes_to_mel", type=str, default=None, metavar="PATH.npy",
                        help="non-streaming only: write the acoustic DVAE's mel [80, 4 x codes] of the generated codes, the segments one after "
                             "the other; needs a checkpoint with acoustic_dvae.* tensors (and an acoustic_dvae_config), or --synthetic")
    args = parser.parse_args()
    if args.decode_codes_to_mel is not None and (args.streaming or args.num_return_sequences != 1):
        raise SystemExit("--decode_codes_to_mel is not on the streaming path (--streaming) and does not combine with --num_return_sequences")
    if args.max_matching_ngram_size is not None and args.prompt_lookup_num_tokens is None:
        raise SystemExit("--max_matching_ngram_size needs --prompt_lookup_num_tokens")
    if args.prompt_lookup_num_tokens is not None:
        if args.streaming:
            raise SystemExit("--prompt_lookup_num_tokens is not on the streaming path (--streaming): GPT.generate serves prompt-lookup "
                             "decoding")
        if args.assistant_layers is not None:
            raise SystemExit("--prompt_lookup_num_tokens and --assistant_layers are two draft sources: pass one of them")
        if not 1 <= args.prompt_lookup_num_tokens <= 15 or not 1 <= (2 if args.max_matching_ngram_size is None
                                                                     else args.max_matching_ngram_size) <= 8:
            raise SystemExit("--prompt_lookup_num_tokens must be in [1, 15] and --max_matching_ngram_size in [1, 8]")
        if (args.num_beams != 1 or args.penalty_alpha is not None or args.num_return_sequences != 1 or args.token_scores is not None
                or (args.guidance_scale is not None and args.guidance_scale != 1.0) or args.sequence_bias or args.bad_words_ids
                or args.forced_eos or args.typical_p is not None or args.epsilon_cutoff is not None or args.eta_cutoff is not None):
            raise SystemExit("--prompt_lookup_num_tokens does not combine with --num_beams, --penalty_alpha, --num_return_sequences, "
                             "--guidance_scale, --token_scores, the warper flags, --sequence_bias, --bad_words_ids or --forced_eos")
    if args.num_assistant_tokens is not None and args.assistant_layers is None:
        raise SystemExit("--num_assistant_tokens needs --assistant_layers")
    if args.assistant_sampling and args.assistant_layers is None and args.prompt_lookup_num_tokens is None:
        raise SystemExit("--assistant_sampling needs --assistant_layers or --prompt_lookup_num_tokens")
    if args.assistant_layers is not None:
        if not args.synthetic:
            raise SystemExit("--assistant_layers needs --synthetic: no draft checkpoint ships with the reference")
        if args.streaming:
            raise SystemExit("--assistant_layers is not on the streaming path (--streaming): GPT.generate serves assisted decoding")
        if args.assistant_layers < 1 or not 1 <= (5 if args.num_assistant_tokens is None else args.num_assistant_tokens) <= 15:
            raise SystemExit("--assistant_layers must be >= 1 and --num_assistant_tokens in [1, 15]")
        if (args.num_beams != 1 or args.penalty_alpha is not None or args.num_return_sequences != 1 or args.token_scores is not None
                or (args.guidance_scale is not None and args.guidance_scale != 1.0) or args.sequence_bias or args.bad_words_ids
                or args.forced_eos or args.typical_p is not None or args.epsilon_cutoff is not None or args.eta_cutoff is not None):
            raise SystemExit("--assistant_layers decodes greedily: it does not combine with --num_beams, --penalty_alpha, "
                             "--num_return_sequences, --guidance_scale, --token_scores, the warper flags, --sequence_bias, --bad_words_ids "
                             "or --forced_eos")
    if args.token_scores is not None:
        if args.streaming:
            raise SystemExit("--token_scores is not on the streaming path (--streaming): GPT.generate serves the per-step scores")
        if args.num_beams != 1 or args.penalty_alpha is not None or args.num_return_sequences != 1:
            raise SystemExit("--token_scores does not combine with --num_beams, --penalty_alpha or --num_return_sequences")
    if args.alignment is not None:
        if args.streaming:
            raise SystemExit("--alignment is not on the streaming path (--streaming): GPT.trace serves the alignment of finished codes")
        if args.num_return_sequences != 1:
            raise SystemExit("--alignment does not combine with --num_return_sequences")
        if args.weights != "fp32":
            raise SystemExit(f"--alignment needs --weights fp32 (the trace pass is a reference-numerics pass), not {args.weights}")
    if args.guidance_scale is not None:
        g = args.guidance_scale
        if g != g or g in (float("inf"), float("-inf")):
            raise SystemExit("--guidance_scale must be finite")
        if g != 1.0 and args.streaming:
            raise SystemExit("--guidance_scale is not on the streaming path (--streaming): classifier-free guidance decodes two KV slots per "
                             "segment, which GPT.generate serves")
        if g != 1.0 and (args.num_beams != 1 or args.penalty_alpha is not None or args.num_return_sequences != 1):
            raise SystemExit("--guidance_scale does not combine with --num_beams, --penalty_alpha or --num_return_sequences")
    if args.negative_ref_audio is not None and (args.guidance_scale is None or args.guidance_scale == 1.0):
        raise SystemExit("--negative_ref_audio needs --guidance_scale (other than 1)")
    if args.num_beams < 1 or (args.streaming and args.num_beams != 1):
        raise SystemExit("--num_beams must be >= 1, and 1 with --streaming")
    if args.num_return_sequences < 1 or (args.num_return_sequences > 1 and (args.streaming or args.penalty_alpha is not None)):
        raise SystemExit("--num_return_sequences must be >= 1, and 1 with --streaming or --penalty_alpha")
    if args.num_beams > 1 and args.num_return_sequences > args.num_beams:
        raise SystemExit("--num_return_sequences must not exceed --num_beams")
    if args.num_beam_groups != 1 or args.diversity_penalty is not None:
        lam = args.diversity_penalty
        if (args.num_beam_groups < 2 or args.num_beams % args.num_beam_groups != 0 or args.num_beam_groups > args.num_beams or lam is None
                or not lam > 0.0 or lam == float("inf") or args.penalty_alpha is not None):
            raise SystemExit("--num_beam_groups must be >= 2 and divide --num_beams, with a finite --diversity_penalty > 0 and without "
                             "--penalty_alpha")
    if args.penalty_alpha is not None:
        if args.streaming or not args.penalty_alpha > 0.0 or args.penalty_alpha == float("inf") or not 2 <= args.top_k <= 16:
            raise SystemExit("--penalty_alpha must be finite and > 0, non-streaming, with --top_k in [2, 16]")
    if args.ras_threshold is not None and not args.ras_window:
        raise SystemExit("--ras_threshold needs --ras_window")
    if args.ras_window is not None:
        if not 0 <= args.ras_window <= 64 or (args.ras_threshold is not None and not 0.0 < args.ras_threshold <= 1.0):
            raise SystemExit("--ras_window must be in 0..64 (0: off) and --ras_threshold in (0, 1]")
        if args.ras_window and (args.num_beams != 1 or args.num_beam_groups != 1 or args.penalty_alpha is not None
                                or args.assistant_layers is not None or args.prompt_lookup_num_tokens is not None):
            raise SystemExit("--ras_window does not combine with --num_beams, --num_beam_groups, --penalty_alpha, --assistant_layers or "
                             "--prompt_lookup_num_tokens: it redraws the token of a sampler step")
    for k in ("presence_penalty", "frequency_penalty"):
        v = getattr(args, k)
        if v is not None and not -2.0 <= v <= 2.0:          # (a NaN fails both comparisons)
            raise SystemExit(f"--{k} must be in [-2, 2], not {v}")
    if args.penalty_window is not None and args.penalty_window < 0:
        raise SystemExit("--penalty_window must be >= 0 (0: every generated code)")
    if (args.presence_penalty or args.frequency_penalty or args.penalty_window) and (
            args.num_beams != 1 or args.num_beam_groups != 1 or args.penalty_alpha is not None or args.assistant_layers is not None
            or args.prompt_lookup_num_tokens is not None):
        raise SystemExit("--presence_penalty / --frequency_penalty / --penalty_window do not combine with --num_beams, --num_beam_groups, "
                         "--penalty_alpha, --assistant_layers or --prompt_lookup_num_tokens: they act in a sampler step")
    wm_cfg = None
    if args.watermark_key is not None:
        import math
        if not 0 <= args.watermark_key < 2 ** 63:
            raise SystemExit(f"--watermark_key must be in [0, 2**63), not {args.watermark_key}")
        if not math.isfinite(args.watermark_bias):
            raise SystemExit(f"--watermark_bias must be finite, not {args.watermark_bias}")
        if not 0.0 < args.watermark_ratio < 1.0:          # (a NaN fails both comparisons)
            raise SystemExit(f"--watermark_ratio must be in (0, 1), not {args.watermark_ratio}")
        if (args.num_beams != 1 or args.num_beam_groups != 1 or args.penalty_alpha is not None or args.assistant_layers is not None
                or args.prompt_lookup_num_tokens is not None or args.ras_window):
            raise SystemExit("--watermark_key does not combine with --num_beams, --num_beam_groups, --penalty_alpha, --assistant_layers, "
                             "--prompt_lookup_num_tokens or --ras_window: the watermark acts in a plain sampler step")
        if args.top_k == 1 and not args.greedy:
            raise SystemExit("--watermark_key with --top_k 1 marks nothing (one candidate survives TopK(1)): pass --greedy for greedy "
                             "search with the mark")
        wm_cfg = dict(greenlist_ratio=args.watermark_ratio, bias=args.watermark_bias, hashing_key=args.watermark_key,
                      seeding_scheme=args.watermark_scheme, context_width=1)
    gen_kw = {k: v for k, v in (("min_new_tokens", args.min_new_tokens), ("no_repeat_ngram_size", args.no_repeat_ngram_size),
                                ("min_p", args.min_p)) if v is not None}
    if args.eos_decay is not None:
        start, factor = args.eos_decay
        if start != int(start):
            raise SystemExit(f"--eos_decay START must be an integer, not {start}")
        gen_kw["exponential_decay_length_penalty"] = (int(start), factor)
    for k, lo_open, hi_open in (("typical_p", True, False), ("epsilon_cutoff", False, True), ("eta_cutoff", False, True)):
        v = getattr(args, k)
        if v is None:
            continue
        # (transformers ignores a cut-off outside (0, 1) and typical_p above 1 without a word: on the command line that is a typo)
        if not ((v > 0.0 if lo_open else v >= 0.0) and (v < 1.0 if hi_open else v <= 1.0)):
            raise SystemExit(f"bad warper flag: --{k} must be in {'(' if lo_open else '['}0, 1{')' if hi_open else ']'}, not {v}")
        gen_kw[k] = v
    for k in ("presence_penalty", "frequency_penalty", "penalty_window"):
        if getattr(args, k):
            gen_kw[k] = getattr(args, k)
    if wm_cfg is not None:
        gen_kw["watermarking_config"] = wm_cfg
    if args.greedy:
        gen_kw["do_sample"] = False
    if args.ras_window:
        gen_kw["ras_window"] = args.ras_window
        if args.ras_threshold is not None:
            gen_kw["ras_threshold"] = args.ras_threshold
    if args.num_beam_groups > 1:
        gen_kw.update(num_beam_groups=args.num_beam_groups, diversity_penalty=args.diversity_penalty)
    if args.sequence_bias or args.bad_words_ids or args.forced_eos:
        if args.streaming or args.num_beams != 1 or args.penalty_alpha is not None:
            raise SystemExit("--sequence_bias, --bad_words_ids and --forced_eos are not on the streaming path (--streaming) and do not combine "
                             "with --num_beams or --penalty_alpha: the sampler paths of GPT.generate serve them")
        try:
            if args.sequence_bias:
                gen_kw["sequence_bias"] = {tuple(int(x) for x in ent.rpartition("=")[0].split(",")): float(ent.rpartition("=")[2])
                                           for ent in args.sequence_bias}
            if args.bad_words_ids:
                gen_kw["bad_words_ids"] = [[int(x) for x in ent.split(",")] for ent in args.bad_words_ids]
        except ValueError:
            raise SystemExit("--sequence_bias takes IDS=VALUE and --bad_words_ids takes IDS, IDS a comma-separated list of codec ids")
        if args.forced_eos:
            gen_kw["forced_eos_token_id"] = 1025
    try:
        from genvc_amd.engine import logits_bias, logits_processors, logits_warpers
        logits_processors(gen_kw, 0, 1026)
        logits_warpers(gen_kw)
        logits_bias(gen_kw, 0, 600, 1026, 1025)      # (any budget above 1: a first-step-only rule must not refuse here)
    except ValueError as e:
        raise SystemExit(f"bad processor flag: {e}")

    if args.synthetic:
        from genvc_amd import config as gcfg
        model, config = model_init_synthetic(gcfg.default_config(tiny=args.tiny, with_acoustic=args.decode_codes_to_mel is not None,
                                                                 resblock_type=args.vocoder_resblock_type),
                                             device=args.device, weight_dtype=args.weights)
    else:
        model, config = model_init(args.model_path, args.device, weight_dtype=args.weights)
        if args.decode_codes_to_mel is not None and (model.acoustic_dvae is None or any(
                k.startswith("acoustic_dvae.") for k in model.missing_checkpoint_keys)):
            raise SystemExit("--decode_codes_to_mel: the checkpoint has no acoustic DVAE (acoustic_dvae_config and acoustic_dvae.* tensors)")
    model.config.top_k = args.top_k
    if args.forced_eos:
        gen_kw["forced_eos_token_id"] = model.gpt.stop_audio_token      # (the flags were validated above against the default vocabulary)
    if args.penalty_alpha is not None:
        gen_kw.update(do_sample=False, penalty_alpha=args.penalty_alpha, top_k=args.top_k)
        if model.gpt.max_slots < args.top_k:           # one KV slot per candidate
            model.gpt.init_gpt_for_inference(max_slots=args.top_k, max_rows=max(4096, 128 * args.top_k), weight_dtype=args.weights)
    if args.num_beams == 1 and model.gpt.max_slots < args.num_return_sequences:     # sampling: one KV slot per candidate
        model.gpt.init_gpt_for_inference(max_slots=args.num_return_sequences, max_rows=max(4096, 128 * args.num_return_sequences),
                                         weight_dtype=args.weights)
    if args.assistant_layers is not None:
        from genvc_amd.inference.model_init import synthetic_assistant
        gen_kw.update(dict(speculative_sampling=True) if args.assistant_sampling else dict(do_sample=False))
        gen_kw.update(num_assistant_tokens=5 if args.num_assistant_tokens is None else args.num_assistant_tokens,
                      assistant_model=synthetic_assistant(model.config, args.assistant_layers, device=args.device,
                                                          max_slots=model.gpt.max_slots, weight_dtype=args.weights))
    if args.prompt_lookup_num_tokens is not None:
        gen_kw.update(dict(speculative_sampling=True) if args.assistant_sampling else dict(do_sample=False))
        gen_kw.update(prompt_lookup_num_tokens=args.prompt_lookup_num_tokens)
        if args.max_matching_ngram_size is not None:
            gen_kw.update(max_matching_ngram_size=args.max_matching_ngram_size)
    src_wav = load_audio(args.src_wav, model.content_sample_rate, device=args.device)
    ref_audio = load_audio(args.ref_audio, model.config.audio.sample_rate, device=args.device)
    if src_wav is None or ref_audio is None:
        raise SystemExit("could not load the input audio")
    guide_kw = {}
    if args.guidance_scale is not None and args.guidance_scale != 1.0:
        guide_kw["guidance_scale"] = args.guidance_scale
        if args.negative_ref_audio is not None:
            neg = load_audio(args.negative_ref_audio, model.config.audio.sample_rate, device=args.device)
            if neg is None:
                raise SystemExit("could not load the negative reference audio")
            guide_kw["negative_ref_audio"] = (neg, model.config.audio.sample_rate)
        if model.gpt.max_slots < 2:                    # two KV slots per segment
            model.gpt.init_gpt_for_inference(max_slots=2, weight_dtype=args.weights)

    if args.num_return_sequences > 1:
        outs = synthesize_utt(model, src_wav, ref_audio, seg_len=args.seg_len, return_details=True, num_beams=args.num_beams,
                              generate_kwargs=gen_kw or None, num_return_sequences=args.num_return_sequences)
        stem, ext = os.path.splitext(args.output_path)
        what = "beam score" if args.num_beams > 1 else "log-probability (raw model distribution)"
        for j, o in enumerate(outs):
            path = f"{stem}_{j}{ext}"
            n = sum(int(c.numel()) for c in o["codes"])
            if o["wav"] is not None and n:
                save_wav(path, o["wav"], config.audio.sample_rate)
            print(f"{path}: {n} codec tokens, {what} {o['score']:.4f}")
        if args.save_tokens:
            torch.save([dict(tokens=torch.cat(o["codes"]).cpu() if o["codes"] else None,
                             latents=None if o["latents"] is None else o["latents"].cpu(), score=o["score"]) for o in outs],
                       args.save_tokens)
    else:
        if args.streaming:
            out = synthesize_utt_streaming(model, src_wav, ref_audio, seg_len=args.seg_len,
                                           stream_chunk_size=args.stream_chunk_size, return_details=True, generate_kwargs=gen_kw or None)
            toks = torch.cat(out["tokens"], 1)
            lat = torch.cat(out["latents"], 1)
        else:
            out = synthesize_utt(model, src_wav, ref_audio, seg_len=args.seg_len, return_details=True, num_beams=args.num_beams,
                                 generate_kwargs=gen_kw or None, token_scores=args.token_scores is not None,
                                 alignment=args.alignment is not None, **guide_kw)
            toks = torch.cat(out["codes"]).unsqueeze(0)
            lat = out["latents"]
            if args.token_scores is not None:
                import numpy as np
                np.savez(args.token_scores, n_segments=len(out["codes"]),
                         **{f"tokens_{i}": c.cpu().numpy() for i, c in enumerate(out["codes"])},
                         **{f"logprobs_{i}": lp.cpu().numpy() for i, lp in enumerate(out["token_logprobs"])})
                print(f"{args.token_scores}: tokens and log-probabilities of {len(out['codes'])} segments")
            if args.alignment is not None:
                import numpy as np
                al = [a.cpu().numpy() for a in out["alignments"]]
                np.savez(args.alignment, n_segments=len(al), **{f"alignment_{i}": a for i, a in enumerate(al)},
                         **{f"argmax_{i}": a.argmax(1) for i, a in enumerate(al)}, **{f"mass_{i}": a.sum(1) for i, a in enumerate(al)})
                print(f"{args.alignment}: alignment of {len(al)} segments, shapes {[a.shape for a in al]}")
        print(f"generated {toks.shape[-1]} codec tokens, latents {tuple(lat.shape)}")
        if args.ras_window:
            print(f"repetition-aware sampling (window {args.ras_window}): redraws per segment {out.get('ras_redraws', [])}")
        if args.decode_codes_to_mel is not None:
            import numpy as np
            dv = model.acoustic_dvae
            segs = [c[c < dv.num_tokens] for c in out["codes"]]
            segs = [c for c in segs if c.numel()]
            dv.bind(max_batch=1, max_frames=4 * max([int(c.numel()) for c in segs] + [1]))
            mels = [dv.decode(c.unsqueeze(0))[0][0].cpu().numpy() for c in segs]
            np.save(args.decode_codes_to_mel, np.concatenate(mels, axis=1) if mels else np.zeros((80, 0), np.float32))
            print(f"{args.decode_codes_to_mel}: acoustic-DVAE mel, frames per segment {[m.shape[1] for m in mels]}")
        if args.assistant_layers is not None:
            st = model.gpt.last_assist_stats
            print(f"assisted decoding, last segment: {int(st['rounds'].sum())} rounds, {int(st['accepted'].sum())} of "
                  f"{int(st['drafted'].sum())} drafts accepted (synthetic weights: chance level)")
        if args.prompt_lookup_num_tokens is not None:
            st = model.gpt.last_assist_stats
            print(f"prompt-lookup decoding, last segment: {int(st['rounds'].sum())} rounds, {int(st['accepted'].sum())} of "
                  f"{int(st['drafted'].sum())} drafts accepted")
        if out["wav"] is not None:
            save_wav(args.output_path, out["wav"], config.audio.sample_rate)
        else:
            print("no vocoder in the model: waveform not written")
        if args.save_tokens:
            torch.save(dict(tokens=toks.cpu(), latents=lat.cpu()), args.save_tokens)
