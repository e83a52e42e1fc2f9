"""`GPT` with the reference's constructor, method names and argument meaning
(/root/reference/layers/gpt.py:87-621) for the inference path.  The module only holds the parameters
(same names and shapes as the reference state dict, so `load_state_dict(ckpt['model'])` works) and
drives libgenvc_hip through `GptEngine`; there is no PyTorch arithmetic fallback.

Mapped entry points: init_gpt_for_inference (:197), get_style_emb (:351, seq_lens included), forward (:375-537: the evaluation pass --
losses, top-10 accuracy, mel logits of a ragged batch -- and return_latent=True), compute_embeddings (:572), generate (:594),
get_generator (:612), inference (:569).
Training mode, return_attentions and eval_sample raise NotImplementedError: out of scope.
"""
import torch
from torch import nn
from torch.nn import functional as F

from .._lib import GenvcHipError
from ..engine import (MAX_ASSISTANT_TOKENS, MAX_LOOKUP_HISTORY, MAX_LOOKUP_NGRAM, MAX_VERIFY_ROWS, AssistedState, BEAM_LENGTH_MODES, beam_early_stopping, check_beam_groups, GroupBeamSearch, MAX_CONTRASTIVE_K, PROC_KWARGS, WARP_KWARGS, BeamSearch, ContrastiveSearch, GptEngine, WarperSets,
                      PENALTY_KWARGS, PenaltyTable, WATERMARK_KWARGS, WatermarkTable, watermark_settings, RAS_KWARGS, RasTable, check_proc_kwargs, logits_bias, logits_penalties,
                      logits_processors, logits_ras, logits_sets, logits_warpers, penalty_settings, ras_counts, sample_params)
from .perceiver_encoder import PerceiverResampler


# Sampled joint / rolling decodes key every row by its own stream (gvc_gpt_generate_rows), so they return the serial path's tokens exactly
# when a row's logits on the rows step do not depend on how many rows share the step.  Measured on the one-launch rows step (d_model 1024):
# they do depend on it (not bit-identical for 5 / 8 / 16 rows), so a near-tie draw can differ from the serial path and the joint sampled
# decode stays opt-in (joint_sampling=True).  tests/test_gpu_row_sampling.py pins this flag to that measurement; DESIGN.md 4.6.
JOINT_SAMPLING_DEFAULT = False


def _no_beams(kw, where):
    """the paths that decode one beam per stream: num_beams > 1 raises, naming the path"""
    if int(kw.get("num_beams", 1) or 1) != 1 or _grouped(kw):
        raise NotImplementedError(f"beam search (num_beams={kw.get('num_beams')}) is not on the {where} path: GPT.generate serves it "
                                  "(the reference streams with num_beams=1 only, inference_utils.py:62,178)")


def _guidance_scale(kw):
    """HF's guidance_scale of the call: None when guidance is off (absent, None or == 1: transformers builds the processor for
    `guidance_scale is not None and guidance_scale != 1` only, generation/utils.py _get_logits_processor), else the scale as a float.
    A bool, a non-number or a non-finite value raises ValueError."""
    s = kw.get("guidance_scale")
    if s is None:
        return None
    if isinstance(s, bool):
        raise ValueError(f"guidance_scale must be a finite number, not {s!r}")
    try:
        v = float(s)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_scale must be a finite number, not {s!r}") from None
    if v != v or v in (float("inf"), float("-inf")):
        raise ValueError(f"guidance_scale must be a finite number, not {s!r}")
    return None if v == 1.0 else v


def _no_guidance(kw, where):
    """the paths that decode one KV slot per stream: classifier-free guidance (guidance_scale != 1) raises, naming the path"""
    s = _guidance_scale(kw)
    if s is not None:
        raise NotImplementedError(f"classifier-free guidance (guidance_scale={s}) is not on the {where} path: GPT.generate serves it "
                                  "(two prefilled KV slots per item, decoded together)")


def _num_return(kw):
    """num_return_sequences of the call (absent or None: 1); below 1 raises ValueError"""
    n = kw.get("num_return_sequences")
    n = 1 if n is None else int(n)
    if n < 1:
        raise ValueError(f"num_return_sequences has to be at least 1, but is {kw.get('num_return_sequences')}")
    return n


def _single_return(kw, where):
    """the paths that keep one row per stream: num_return_sequences > 1 raises, naming the path"""
    if _num_return(kw) != 1:
        raise NotImplementedError(f"num_return_sequences={kw.get('num_return_sequences')} is not on the {where} path: GPT.generate serves "
                                  "it (one prefill per item, fanned out to the candidates' KV slots)")


def _sample_return_kwargs(kw, B=None, max_slots=None):
    """num_return_sequences = N of a call that is neither contrastive nor beam search, validated: N > 1 needs sampling (ValueError for
    greedy decoding, as HF raises it); with B and max_slots given, B * N > max_slots raises ValueError.  -> N"""
    N = _num_return(kw)
    if N > 1 and not kw.get("do_sample", True):
        raise ValueError(f"num_return_sequences has to be 1, but is {N} when doing greedy search")
    if N > 1 and B is not None and max_slots is not None and B * N > max_slots:
        raise ValueError(f"sampling {N} sequences for each of {B} items needs {B * N} KV slots; the context has {max_slots} "
                         "(init_gpt_for_inference(max_slots=...))")
    return N


def _beam_kwargs(kw):
    """the modes of HF generate(num_beams > 1) this build does not serve raise NotImplementedError, naming the mode; returns the
    (K, length_penalty, repetition_penalty, beam_length_mode) of a deterministic beam search.  num_return_sequences outside [1, K] and an
    early_stopping other than False, True or "never" raise ValueError (HF's rules); _beam_returns gives the two"""
    K = int(kw.get("num_beams", 1) or 1)
    _beam_groups(kw)
    if kw.get("do_sample", True):
        raise NotImplementedError(f"beam sampling (do_sample=True, num_beams={K}) is not implemented: deterministic beam search needs "
                                  "do_sample=False")
    if kw.get("constraints") or kw.get("force_words_ids"):
        raise NotImplementedError("constrained beam search (constraints, force_words_ids) is not implemented")
    _beam_returns(kw)
    mode = kw.get("beam_length_mode", "4.33")
    if mode not in BEAM_LENGTH_MODES:
        raise ValueError(f"beam_length_mode must be one of {sorted(BEAM_LENGTH_MODES)}, not {mode!r}")
    return K, float(kw.get("length_penalty", 1.0)), float(kw.get("repetition_penalty", 1.0)), mode


def _grouped(kw):
    """the call names group beam search: num_beam_groups other than 1, or a diversity_penalty other than 0"""
    g, lam = kw.get("num_beam_groups"), kw.get("diversity_penalty")
    return (g is not None and int(g) != 1) or (lam is not None and float(lam) != 0.0)


def _beam_groups(kw):
    """(num_beam_groups, diversity_penalty) of a beam search, (1, 0.0) without groups; validated as HF validates them (ValueError:
    do_sample=True with groups, K % G != 0, G > K, a diversity_penalty that is not finite and >= 0 or is positive with G == 1, a
    non-default typical_p -- the reference's dispatcher, layers/stream_generator.py:522-524).  G > 1 without a positive
    diversity_penalty is NotImplementedError: the groups would all run the same search."""
    if not _grouped(kw):
        return 1, 0.0
    K = int(kw.get("num_beams", 1) or 1)
    G = 1 if kw.get("num_beam_groups") is None else int(kw["num_beam_groups"])
    lam = 0.0 if kw.get("diversity_penalty") is None else float(kw["diversity_penalty"])
    if kw.get("do_sample", True):
        raise ValueError("`diversity_penalty` / `num_beam_groups` is not a valid argument when `do_sample=True`: group beam search is "
                         "deterministic")
    K, G, lam = check_beam_groups(K, G, lam)
    typ = kw.get("typical_p")
    if typ is not None and float(typ) != 1.0:
        raise ValueError("Decoder argument `typical_p` is not supported with beam groups.")
    if lam == 0.0:
        raise NotImplementedError(f"group beam search (num_beam_groups={G}) without a positive diversity_penalty is not implemented: "
                                  "identical groups are not served")
    return G, lam


def _beam_returns(kw):
    """(num_return_sequences, early_stopping) of a beam search, validated as HF validates them"""
    K = int(kw.get("num_beams", 1))
    N = _num_return(kw)
    if N > K:
        raise ValueError(f"`num_return_sequences` ({N}) has to be smaller or equal to `num_beams` ({K}).")
    early = kw.get("early_stopping", False)
    beam_early_stopping(early)
    return N, early


def _contrastive_mode(kw):
    """HF 4.33's contrastive-search test, which takes precedence over num_beams: top_k > 1, do_sample=False, penalty_alpha > 0 -> (K,
    penalty_alpha), else None.  top_k absent is GenerationConfig's 50; an explicit top_k=None fails the test (GenerationConfig.update
    keeps the None), so such a call decodes greedily as in 4.33.  A non-finite penalty_alpha raises ValueError.  do_sample=True with
    penalty_alpha stays sampling (4.33 ignores the alpha)."""
    alpha = kw.get("penalty_alpha")
    if alpha is None or kw.get("do_sample", True) is not False:
        return None
    K = kw["top_k"] if "top_k" in kw else 50
    if K is None or int(K) <= 1:
        return None
    alpha = float(alpha)
    if alpha != alpha or alpha in (float("inf"), float("-inf")):
        raise ValueError(f"penalty_alpha must be finite, not {kw.get('penalty_alpha')!r}")
    if alpha <= 0.0:
        return None
    return int(K), alpha


def _contrastive_kwargs(kw, B=None, max_slots=None):
    """_contrastive_mode, validated for the device: None when the kwargs do not select contrastive search, else (K, penalty_alpha,
    repetition_penalty).  num_return_sequences > 1 raises ValueError (4.33 raises it), K > 16 NotImplementedError; with B and
    max_slots given, B * K > max_slots raises ValueError."""
    mode = _contrastive_mode(kw)
    if mode is None:
        return None
    K, alpha = mode
    if int(kw.get("num_return_sequences", 1) or 1) > 1:
        raise ValueError(f"num_return_sequences has to be 1, but is {kw.get('num_return_sequences')} when doing contrastive search")
    if K > MAX_CONTRASTIVE_K:
        raise NotImplementedError(f"contrastive search with top_k={K} is not implemented: the device ranks at most {MAX_CONTRASTIVE_K} "
                                  "candidates per step")
    if B is not None and max_slots is not None and B * K > max_slots:
        raise ValueError(f"contrastive search over {B} items x {K} candidates needs {B * K} KV slots; the context has {max_slots} "
                         "(init_gpt_for_inference(max_slots=...))")
    return K, alpha, float(kw.get("repetition_penalty", 1.0))


def _no_contrastive(kw, where):
    """the paths that decode one row per stream: the contrastive-search kwargs raise, naming the path (before any check of K)"""
    if _contrastive_mode(kw) is not None:
        raise NotImplementedError(f"contrastive search (penalty_alpha={kw.get('penalty_alpha')}, top_k={kw.get('top_k', 50)}, "
                                  f"do_sample=False) is not on the {where} path: GPT.generate serves it (the reference's streaming "
                                  "harness always samples, inference_utils.py:178)")


# refused by name on the paths that return bare tokens.  output_hidden_states is not among them: the reference's streaming harness passes
# output_hidden_states=True to get_generator as its way of asking for the latents (inference_utils.py:178), which these paths yield
# anyway; as a request for a result object's `hidden_states` it only means something with return_dict_in_generate, which is refused
OUTPUT_KWARGS = ("return_dict_in_generate", "output_scores", "output_logits", "output_attentions")
MAX_TRACE_BYTES = 2 << 30          # default of generate(max_trace_bytes=): the attentions tensor of one call


class GenerateOutput(dict):
    """what GPT.generate(return_dict_in_generate=True) returns, read as attributes or by key (HF's ModelOutput habit):
    sequences  int64 [rows, n]: what the call returns without the kwarg
    scores     output_scores=True: a tuple of n fp32 [rows, V] views into one device tensor, scores[t] the row step t decoded from as
               transformers' logits processors (and, when sampling, warpers) leave it; else None
    logits     output_logits=True: likewise the raw head output of every step (under guidance the conditional row); else None
    latents    `last_latents` of the call
    sequences_scores  beam search: `last_beam_scores`; else None
    attentions output_attentions=True: HF's form, a tuple over the n steps of tuples over the L layers of fp32 views into one device
               tensor [L, rows, H, T, T] (T = P + n, P the prefix rows): step 0 [rows, H, P+1, P+1], step i [rows, H, 1, P+1+i]; else
               None.  A step at or past a row's end (HF ran it on a pad token) is all zeros.
    hidden_states  output_hidden_states=True: likewise L + 1 entries per step (the embeddings, each layer's output, ln_f of the last
               one), views into [L+1, rows, T, D]: step 0 [rows, P+1, D], step i [rows, 1, D]; else None
    Both keys exist only in the result of a call that asked for either (the other one is then None): a result without them reads as it
    always has (AttributeError / KeyError).
    GPT.trace fills the same object with the full tensors under `attentions` / `hidden_states` and `alignment` [B, n, Tc]."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


def _output_kwargs(kw):
    """(return_dict_in_generate, output_scores, output_logits) of the call as HF reads them: without return_dict_in_generate the
    call returns the bare tensor and the other two are ignored"""
    rd = bool(kw.get("return_dict_in_generate"))
    return rd, rd and bool(kw.get("output_scores")), rd and bool(kw.get("output_logits"))


def _no_outputs(kw, where):
    """the paths that return bare tokens: return_dict_in_generate / output_scores / output_logits / output_attentions raise, naming the
    path (output_hidden_states alone keeps its old treatment, see OUTPUT_KWARGS)"""
    for k in OUTPUT_KWARGS:
        if kw.get(k):
            raise NotImplementedError(f"{k}={kw.get(k)!r} is not on the {where} path: GPT.generate serves it (one result object per "
                                      "call, per-step scores, attentions and hidden states of the sampler paths)")


def _trace_kwargs(kw):
    """(output_attentions, output_hidden_states) of the call as HF reads them: ignored without return_dict_in_generate"""
    rd = bool(kw.get("return_dict_in_generate"))
    return rd and bool(kw.get("output_attentions")), rd and bool(kw.get("output_hidden_states"))


def _no_trace(kw, mode):
    """the modes of GPT.generate without the trace pass: output_attentions / output_hidden_states raise, naming the mode"""
    at, hs = _trace_kwargs(kw)
    if at or hs:
        which = "output_attentions" if at else "output_hidden_states"
        raise NotImplementedError(f"{which}=True with {mode} is not implemented: the trace pass follows one token row per prompt row "
                                  "(greedy, sampling, num_return_sequences, guidance_scale); GPT.trace serves any finished ids")


def _trace_bytes_check(L, rows, H, T, limit):
    """the size guard of output_attentions: the [L, rows, H, T, T] fp32 tensor against max_trace_bytes"""
    size = 4 * L * rows * H * T * T
    if size > limit:
        raise ValueError(f"output_attentions: {L} layers x {rows} rows x {H} heads x {T}^2 fp32 weights are {size} bytes "
                         f"({size / 2 ** 30:.2f} GiB), above max_trace_bytes={limit}: raise it, or take "
                         "GPT.trace(..., output_attentions=False) for the hidden states and the alignment (one layer's weights at a time)")


def _no_step_outputs(kw, mode):
    """the modes of GPT.generate without per-step scores: output_scores / output_logits raise, naming the mode (return_dict_in_generate
    alone is served)"""
    _, sc, lg = _output_kwargs(kw)
    if sc or lg:
        which = "output_scores" if sc else "output_logits"
        raise NotImplementedError(f"{which}=True with {mode} is not implemented: HF's scores of that mode are not the sampler's rows "
                                  "(beam scores add the running beam score and need beam_indices); return_dict_in_generate=True alone is "
                                  "served")


# the BIAS_KWARGS (engine.logits_bias) that change a call; forced_bos_token_id never does (see GPT.generate)
_BIAS_ON = ("sequence_bias", "bad_words_ids", "forced_eos_token_id", "renormalize_logits")


def _no_bias(kw, where):
    """the modes and paths the call-wide sequence bias does not serve: sequence_bias / bad_words_ids / forced_eos_token_id /
    renormalize_logits at anything but an off spelling (None, {}, [], False) raise, naming the kwarg and the mode or path"""
    for k in _BIAS_ON:
        v = kw.get(k)
        if v is None or v is False or (isinstance(v, (dict, list, tuple)) and len(v) == 0):
            continue
        raise NotImplementedError(f"{k}={v!r} is not served with {where}: GPT.generate serves it on the sampler paths (greedy, sampling, "
                                  "num_return_sequences, guidance_scale), one call-wide set per call")


def _ras_on(kw):
    """the call asks for repetition-aware sampling (engine.RAS_KWARGS; ras_window None or 0 is off).  ValueError: malformed settings
    (engine.ras_counts), and do_sample=False -- greedy search has no distribution to draw again from; "greedy with an escape" is
    do_sample=True with top_k=1, whose redraw runs at the call's temperature"""
    if ras_counts(kw) is None:
        return False
    if not kw.get("do_sample", True):
        raise ValueError(f"ras_window={kw.get('ras_window')} with do_sample=False: greedy search has nothing to draw again from; pass "
                         "do_sample=True with top_k=1 (the argmax, redrawn from the full distribution when it repeats)")
    return True


def _no_ras(kw, mode):
    """the modes of GPT.generate that repetition-aware sampling does not serve raise, naming the combination (whatever do_sample is:
    most of them are greedy modes)"""
    if ras_counts(kw) is not None:
        raise NotImplementedError(f"ras_window={kw.get('ras_window')} with {mode} is not implemented: repetition-aware sampling redraws "
                                  "the token of a sampler step (greedy at top_k=1, sampling, num_return_sequences, guidance_scale)")


def _no_penalties(kw, mode):
    """the modes of GPT.generate that the presence / frequency / windowed penalties do not serve raise, naming the kwarg and the mode
    (malformed settings: ValueError, engine.penalty_settings)"""
    if penalty_settings(kw) is not None:
        k = next(k for k in PENALTY_KWARGS if kw.get(k))
        raise NotImplementedError(f"{k}={kw.get(k)} with {mode} is not implemented: the presence / frequency / windowed repetition "
                                  "penalties act in a sampler step (greedy, sampling, num_return_sequences, guidance_scale)")


def _watermark(kw, vocab):
    """the watermarking_config of a sampler-step call (GPT.generate: greedy search, sampling, num_return_sequences, guidance_scale;
    get_generator) -> engine.WatermarkSettings, or None when it is off.  Malformed settings: ValueError / NotImplementedError
    (engine.watermark_settings).  The combinations that cannot carry transformers' semantics raise instead of leaving the output
    unmarked:
    do_sample=True with top_k=1: ValueError -- after TopK(1) one entry survives, so the mark behind the warpers cannot move a token; a
    marked greedy stream is do_sample=False;
    selfhash under greedy search: NotImplementedError (the argmax path has no 40 highest scores);
    selfhash with typical_p: NotImplementedError (typical decoding may drop the highest scores: its survivors do not lead the order);
    ras_window: NotImplementedError (a redraw from the untruncated row would need a rule of its own)."""
    s = watermark_settings(kw, vocab)
    if s is None:
        return None
    sampling = kw.get("do_sample", True)
    if sampling and kw.get("top_k", 0) == 1:
        raise ValueError("watermarking_config with do_sample=True and top_k=1: TopK(1) leaves one candidate, so the watermark (behind "
                         "the warpers, as in transformers) could not move a single token; pass do_sample=False for greedy search "
                         "with the mark")
    if not sampling and s.seeding_scheme == "selfhash":
        raise NotImplementedError("watermarking_config with seeding_scheme='selfhash' and do_sample=False (greedy search) is not "
                                  "implemented: the argmax path has no 40 highest scores to restrict the bias to; use 'lefthash'")
    tp = kw.get("typical_p")
    if s.seeding_scheme == "selfhash" and tp is not None and tp < 1.0:
        raise NotImplementedError(f"watermarking_config with seeding_scheme='selfhash' and typical_p={tp} is not implemented: typical "
                                  "decoding can drop the highest scores, so the 40 highest survivors are no prefix of the sorted row")
    if ras_counts(kw) is not None:
        raise NotImplementedError(f"watermarking_config with ras_window={kw.get('ras_window')} is not implemented: the redraw from the "
                                  "untruncated row would need a rule of its own")
    return s


def _no_watermark(kw, mode, vocab):
    """the modes and paths that do not carry the watermark raise, naming the kwarg and the mode: an unmarked output must never be
    silent (malformed settings: engine.watermark_settings)"""
    if watermark_settings(kw, vocab) is not None:
        raise NotImplementedError(f"watermarking_config with {mode} is not implemented: the watermark acts in a sampler step of "
                                  "GPT.generate (greedy search, sampling, num_return_sequences, guidance_scale), get_generator and the "
                                  "sampled rows of generate_groups / generate_rolling / StreamSessions")


def _watermark_rows(kw, items, where, vocab):
    """the joint paths (generate_groups, generate_rolling; `items`: the merged per-item dicts or None): a mark, call-wide or on any
    item, is served on sampled rows.  Greedy rows (top_k=1 or do_sample=False) raise NotImplementedError naming the path -- their
    kernel adds the bias behind the division by the call's temperature, which is greedy search only at temperature 1 --: GPT.generate(
    do_sample=False) serves greedy search with the mark.  The refused combinations of _watermark raise as they do there.
    -> whether any mark is on"""
    on = False
    for d in ([kw] if items is None else [dict(kw, **(d or {})) for d in items]):
        if watermark_settings(d, vocab) is None:
            continue
        on = True
        if kw.get("top_k", 0) == 1 or not kw.get("do_sample", True):
            raise NotImplementedError(f"watermarking_config with greedy rows (top_k=1 or do_sample=False) on {where} is not "
                                      "implemented: GPT.generate(do_sample=False) serves greedy search with the mark")
        _watermark(d, vocab)
    return on


ASSIST_KWARGS = ("assistant_model", "num_assistant_tokens", "num_assistant_tokens_schedule", "assistant_cond_latents",
                 "speculative_sampling")


LOOKUP_KWARGS = ("prompt_lookup_num_tokens", "max_matching_ngram_size")
_LOOKUP_MODE = "prompt-lookup decoding (prompt_lookup_num_tokens)"


def _no_assistant(kw, where):
    """the paths without assisted decoding: assistant_model and prompt_lookup_num_tokens raise, naming the path"""
    if kw.get("assistant_model") is not None:
        raise NotImplementedError(f"assisted decoding (assistant_model) is not on the {where} path: GPT.generate serves it (greedy, "
                                  "one draft context next to the target's)")
    if kw.get("prompt_lookup_num_tokens") is not None or kw.get("max_matching_ngram_size") is not None:
        raise NotImplementedError(f"{_LOOKUP_MODE} is not on the {where} path: GPT.generate serves it (rounds of one verification "
                                  "pass over the call's own rows)")


def _lookup(kw):
    """the call asks for prompt-lookup decoding.  ValueError: the kwarg next to assistant_model (two draft sources), and
    max_matching_ngram_size without it (HF ignores the orphan; here a typo in the other kwarg would silently decode plainly)"""
    if kw.get("prompt_lookup_num_tokens") is None:
        if kw.get("max_matching_ngram_size") is not None:
            raise ValueError(f"max_matching_ngram_size={kw.get('max_matching_ngram_size')!r} needs prompt_lookup_num_tokens")
        return False
    if kw.get("assistant_model") is not None:
        raise ValueError("prompt_lookup_num_tokens and assistant_model are two draft sources: pass one of them")
    return True


def _speculative(kw):
    """an assisted call that samples: the opt-in kwarg, do_sample (default True) and a top_k that leaves a choice.  do_sample=False or
    top_k=1 with the kwarg is the greedy mode"""
    return bool(kw.get("speculative_sampling")) and bool(kw.get("do_sample", True)) and kw.get("top_k", 0) != 1


def _assisted_kwargs(kw, B, lookup=False):
    """the kwargs of GPT.generate(assistant_model=...) validated -> k, the drafts per round.  Assisted decoding is greedy, or -- with
    the opt-in speculative_sampling=True -- sampled (do_sample, top_k != 1: _speculative(kw)): every other mode of generate raises
    NotImplementedError naming the combination; a k outside [1, 15], more than 128 verification rows and a schedule other than
    "constant" raise ValueError.
    lookup: the kwargs of GPT.generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=N) instead -> (k, N): the same refusals
    under that mode's name, k required in [1, 15], N in [1, 8] (default 2, HF's)"""
    mode = _LOOKUP_MODE if lookup else "assisted decoding (assistant_model)"
    spec = kw.get("speculative_sampling")
    if spec is not None and not isinstance(spec, bool):
        raise ValueError(f"speculative_sampling must be True, False or None, not {spec!r}")
    if _guidance_scale(kw) is not None:
        raise NotImplementedError(f"guidance_scale={kw.get('guidance_scale')} with {mode} is not implemented")
    if _contrastive_mode(kw) is not None:
        raise NotImplementedError(f"contrastive search (penalty_alpha={kw.get('penalty_alpha')}) with {mode} is not implemented")
    if _grouped(kw):
        raise NotImplementedError(f"beam groups (num_beam_groups / diversity_penalty) with {mode} are not implemented")
    if int(kw.get("num_beams", 1) or 1) != 1:
        raise NotImplementedError(f"beam search (num_beams={kw.get('num_beams')}) with {mode} is not implemented")
    if _num_return(kw) != 1:
        raise NotImplementedError(f"num_return_sequences={kw.get('num_return_sequences')} with {mode} is not implemented")
    if kw.get("do_sample", True) and kw.get("top_k", 0) != 1 and not spec:
        raise NotImplementedError(f"sampling (do_sample=True, top_k={kw.get('top_k', 0)}) with {mode} is not implemented: speculative "
                                  "sampling needs the draft's warped rows; pass do_sample=False or top_k=1 (or opt in with "
                                  "speculative_sampling=True)")
    _no_step_outputs(kw, mode)
    _no_trace(kw, mode)
    _no_bias(kw, mode)
    if logits_warpers(kw, sampling=_speculative(kw)) is not None:
        raise NotImplementedError(f"typical_p / epsilon_cutoff / eta_cutoff with {mode} are not implemented")
    sched = kw.get("num_assistant_tokens_schedule", "constant")
    if sched is not None and sched != "constant":
        raise ValueError(f"num_assistant_tokens_schedule={sched!r} with {mode}: only \"constant\" is served (a heuristic schedule needs "
                         "a host round trip per round)")
    name = "prompt_lookup_num_tokens" if lookup else "num_assistant_tokens"
    k = kw.get(name)
    k = 5 if k is None else k          # (a lookup call always names its k: _lookup)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_ASSISTANT_TOKENS:
        raise ValueError(f"{name} must be an int in [1, {MAX_ASSISTANT_TOKENS}] for {mode}, not {k!r}")
    if B * (k + 1) > MAX_VERIFY_ROWS:
        raise ValueError(f"{mode}: {B} items x ({name} + 1 = {k + 1}) rows exceed the {MAX_VERIFY_ROWS} rows of one "
                         "verification pass")
    if not lookup:
        return k
    N = kw.get("max_matching_ngram_size")
    N = 2 if N is None else N
    if isinstance(N, bool) or not isinstance(N, int) or not 1 <= N <= MAX_LOOKUP_NGRAM:
        raise ValueError(f"max_matching_ngram_size must be an int in [1, {MAX_LOOKUP_NGRAM}] for {mode}, not {N!r}")
    return k, N


def _plain_rows_only(kw, where, beams=True):
    """the paths that decode one sampled or greedy row per stream and return bare tokens (grouped, rolling, streaming, sessions):
    every mode only GPT.generate serves raises, naming the path `where`.  beams=False: the caller has no num_beams to refuse"""
    if beams:
        _no_beams(kw, where)
    _no_contrastive(kw, where)
    _single_return(kw, where)
    _no_guidance(kw, where)
    _no_outputs(kw, where)
    _no_bias(kw, f"the {where} path")
    _no_assistant(kw, where)


def _step_views(probs, hidden, P, n):
    """the full tensors of a trace pass (probs [L, rows, H, T, T], hidden [L+1, rows, T, D], either None) cut into HF's per-step form:
    tuples over the n steps of tuples over the layers of views -- step 0 the P + 1 prompt rows, step i the one row P + i"""
    def cut(t, f):
        return None if t is None else tuple(tuple(f(t[l], 0 if i == 0 else P + i, P + i + 1) for l in range(t.shape[0])) for i in range(n))
    return cut(probs, lambda p, lo, hi: p[:, :, lo:hi, :hi]), cut(hidden, lambda h, lo, hi: h[:, lo:hi])


def _generate_call(eng, *args, **kw):
    """eng.generate_call(...); an engine stand-in without one gets GptEngine's, over the entries it does have"""
    fn = getattr(eng, "generate_call", None)
    return fn(*args, **kw) if fn is not None else GptEngine.generate_call(eng, *args, **kw)


def _any_proc(kw):
    """a processor kwarg is given (engine.logits_processors may still find every one at its default)"""
    return any(kw.get(k) is not None for k in PROC_KWARGS)


def _proc_arg(proc):
    """the engine call's processor argument: none at all without processors (the call is exactly the one without them)"""
    return {} if proc is None else {"proc": proc}


def _per_item_procs(kw, item_kwargs, n, name, vocab):
    """group_kwargs / job_kwargs: one processor dict (or None) per item, merged over the call-wide processor and warper kwargs of `kw`
    -> the merged dict of every item.  Keys other than PROC_KWARGS / WARP_KWARGS, a wrong count and malformed settings raise
    ValueError naming the item."""
    item_kwargs = list(item_kwargs)
    if len(item_kwargs) != n:
        raise ValueError(f"{name}: {len(item_kwargs)} processor dicts for {n} items")
    base = {k: kw[k] for k in PROC_KWARGS + WARP_KWARGS + RAS_KWARGS + PENALTY_KWARGS + WATERMARK_KWARGS if kw.get(k) is not None}
    out = []
    for i, d in enumerate(item_kwargs):
        check_proc_kwargs(d, f"{name}[{i}]")
        m = dict(base, **(d or {}))
        try:
            logits_processors(m, 0, vocab)
            logits_warpers(m, sampling=kw.get("do_sample", True))
            _ras_on(dict(m, do_sample=kw.get("do_sample", True)))
            penalty_settings(m)
            watermark_settings(m, vocab)
        except ValueError as e:
            raise ValueError(f"{name}[{i}]: {e}") from None
        out.append(m)
    return out


class _Holder(nn.Module):
    pass


def _p(*shape, std=0.02, ones=False):
    t = torch.ones(*shape) if ones else torch.empty(*shape).normal_(std=std) if std else torch.zeros(*shape)
    return nn.Parameter(t, requires_grad=False)


class LearnedPositionEmbeddings(nn.Module):
    """holds `emb.weight` [seq_len, dim] (reference gpt.py:21-40)"""

    def __init__(self, seq_len, model_dim, init=0.02):
        super().__init__()
        self.emb = _Holder()
        self.emb.weight = _p(seq_len, model_dim, std=init)
        self.seq_len = seq_len


def _conv1d(nin, nout):
    m = _Holder()
    m.weight = _p(nin, nout)            # HF Conv1D layout [in, out]
    m.bias = _p(nout, std=0)
    return m


def _ln(d):
    m = _Holder()
    m.weight = _p(d, ones=True)
    m.bias = _p(d, std=0)
    return m


def perceiver_key_mask(seq_lens, n_frames, num_latents=32):
    """the Perceiver mask of reference gpt.py:362-367, bool [B, n_frames + num_latents]: cat([frame j < seq_lens[b], ones(num_latents)]).
    The reference's Attention lays its keys out as cat([latents, frames]) (perceiver_encoder.py:310-311), so entry j of this mask meets
    key j of [latents | frames]: the masked keys are those with index in [len, n_frames) -- frames len - num_latents .. n_frames -
    num_latents - 1, and latents len .. num_latents - 1 when len < num_latents -- and the last num_latents frames are always attended.
    That misalignment is the reference's behaviour and is reproduced, not repaired."""
    seq_lens = torch.as_tensor(seq_lens).to("cpu", torch.long).reshape(-1)
    frames = torch.arange(int(n_frames)).unsqueeze(0) < seq_lens.unsqueeze(1)
    return torch.cat([frames, torch.ones(seq_lens.shape[0], num_latents, dtype=torch.bool)], dim=-1)


def forward_eval_prepare(text_inputs, text_lengths, audio_codes, wav_lengths, *, code_stride_len=1024, start_text_token=256,
                         stop_text_token=257, start_audio_token=1024, stop_audio_token=1025, number_text_tokens=258,
                         num_audio_tokens=1026, n_cond=32):
    """The integer preparation of GPT.forward (reference gpt.py:404-474, 514-518) on the host, as CPU int64 / bool tensors:
      text_ids [B, Lt]      = start | text[:max(text_lengths)] with stop from each row's length on | stop          (Lt = max len + 2)
      code_ids [B, Lm]      = start | codes zero-padded to max(code_lengths) with stop from each row's real length on | stop
                              (code_lengths = ceil(wav_lengths / code_stride_len) + 3, Lm = max(code_lengths) + 2)
      text_targets / mel_targets = the same rows without the start token and with one more stop, -1 from position l + 1 on
                              (l = the row's text length / code length with its + 3)
      key_mask [B, n_cond + Lt + Lm] = ones over the conditioning rows; text and code positions > l are 0 (the first stop token of a
                              text row is itself a masked key)."""
    text_inputs = torch.as_tensor(text_inputs).to("cpu", torch.long)
    audio_codes = torch.as_tensor(audio_codes).to("cpu", torch.long)
    text_lengths = torch.as_tensor(text_lengths).to("cpu", torch.long).reshape(-1)
    wav_lengths = torch.as_tensor(wav_lengths).to("cpu").reshape(-1)
    B = text_inputs.shape[0]
    if text_inputs.ndim != 2 or audio_codes.ndim != 2 or audio_codes.shape[0] != B or text_lengths.shape[0] != B or wav_lengths.shape[0] != B:
        raise ValueError(f"forward: text {tuple(text_inputs.shape)}, codes {tuple(audio_codes.shape)}, {text_lengths.shape[0]} text lengths "
                         f"and {wav_lengths.shape[0]} wav lengths do not describe one batch")
    if int(text_lengths.min()) < 0 or int(wav_lengths.min()) < 0:
        raise ValueError("forward: negative length")
    max_text_len = int(text_lengths.max())
    code_lengths = torch.ceil(wav_lengths / code_stride_len).long() + 3                      # gpt.py:405
    max_mel_len = int(code_lengths.max())
    if max_mel_len > audio_codes.shape[-1]:
        audio_codes = F.pad(audio_codes, (0, max_mel_len - audio_codes.shape[-1]))           # :413-414
    if max_text_len > text_inputs.shape[-1]:
        raise ValueError(f"forward: max(text_lengths) {max_text_len} > text_inputs.shape[-1] {text_inputs.shape[-1]}")      # :420-422
    if text_inputs.numel() and (int(text_inputs.min()) < 0 or int(text_inputs.max()) >= number_text_tokens):
        raise ValueError(f"forward: text ids outside [0, {number_text_tokens})")
    if int(audio_codes.min()) < 0 or int(audio_codes.max()) >= num_audio_tokens:
        raise ValueError(f"forward: audio codes outside [0, {num_audio_tokens})")
    text = F.pad(text_inputs[:, :max_text_len], (0, 1), value=stop_text_token)               # :425
    codes = F.pad(audio_codes[:, :max_mel_len], (0, 1), value=stop_audio_token)              # :430
    for b in range(B):                                                                       # set_text_padding / set_mel_padding, :237-260
        lt, lc = int(text_lengths[b]), int(code_lengths[b]) - 3
        if lt < text.shape[-1]:
            text[b, lt:] = stop_text_token
        if lc < codes.shape[-1]:
            codes[b, lc:] = stop_audio_token
    text_ids, text_targets = F.pad(text, (1, 0), value=start_text_token), F.pad(text, (0, 1), value=stop_text_token)        # :232-235
    code_ids, mel_targets = F.pad(codes, (1, 0), value=start_audio_token), F.pad(codes, (0, 1), value=stop_audio_token)
    mask_text = torch.ones(text_ids.shape, dtype=torch.bool)
    mask_mel = torch.ones(code_ids.shape, dtype=torch.bool)
    for b in range(B):                                                                       # :470-474, 514-518
        lt, lc = int(text_lengths[b]), int(code_lengths[b])
        mask_text[b, lt + 1:] = False
        mask_mel[b, lc + 1:] = False
        text_targets[b, lt + 1:] = -1
        mel_targets[b, lc + 1:] = -1
    key_mask = torch.cat([torch.ones(B, n_cond, dtype=torch.bool), mask_text, mask_mel], dim=1)
    return dict(text_ids=text_ids, text_targets=text_targets, code_ids=code_ids, mel_targets=mel_targets, key_mask=key_mask,
                code_lengths=code_lengths)


class GPT(nn.Module):
    rolling_samples = True          # generate_rolling samples with per-job keys (job_seeds): parallel_offline rolls sampled runs too

    def __init__(self, start_text_token=256, stop_text_token=257, layers=8, model_dim=512, heads=8,
                 max_text_tokens=120, max_mel_tokens=250, max_prompt_tokens=70, max_conditioning_inputs=1,
                 code_stride_len=1024, number_text_tokens=258, num_audio_tokens=1026, start_audio_token=1024,
                 stop_audio_token=1025, train_solo_embeddings=False, checkpointing=False,
                 average_conditioning_embeddings=False, fix_condition_embeddings=False, label_smoothing=0.0,
                 perceiver_cond_length_compression=256):
        super().__init__()
        self.number_text_tokens = number_text_tokens
        self.start_text_token, self.stop_text_token = start_text_token, stop_text_token
        self.num_audio_tokens = num_audio_tokens
        self.start_audio_token, self.stop_audio_token = start_audio_token, stop_audio_token
        self.layers, self.heads, self.model_dim = layers, heads, model_dim
        self.max_conditioning_inputs = max_conditioning_inputs
        self.max_gen_mel_tokens = max_mel_tokens - max_conditioning_inputs - 2             # gpt.py:131
        self.max_mel_tokens = max_mel_tokens + 2 + max_conditioning_inputs                 # :132
        self.max_text_tokens = max_text_tokens + 2                                         # :133
        self.max_prompt_tokens = max_prompt_tokens
        self.code_stride_len = code_stride_len
        self.label_smoothing = label_smoothing
        self.perceiver_cond_length_compression = perceiver_cond_length_compression
        self.train_solo_embeddings = train_solo_embeddings
        self.average_conditioning_embeddings = average_conditioning_embeddings

        d = model_dim
        self.text_embedding = _Holder(); self.text_embedding.weight = _p(number_text_tokens, d)
        self.mel_embedding = _Holder(); self.mel_embedding.weight = _p(num_audio_tokens, d)
        self.mel_pos_embedding = LearnedPositionEmbeddings(self.max_mel_tokens, d)
        self.text_pos_embedding = LearnedPositionEmbeddings(self.max_text_tokens, d)
        self.gpt = _Holder()
        self.gpt.h = nn.ModuleList()
        for _ in range(layers):
            blk = _Holder()
            blk.ln_1, blk.ln_2 = _ln(d), _ln(d)
            blk.attn = _Holder(); blk.attn.c_attn = _conv1d(d, 3 * d); blk.attn.c_proj = _conv1d(d, d)
            blk.mlp = _Holder(); blk.mlp.c_fc = _conv1d(d, 4 * d); blk.mlp.c_proj = _conv1d(4 * d, d)
            self.gpt.h.append(blk)
        self.gpt.ln_f = _ln(d)
        self.final_norm = _ln(d)
        self.text_head = _Holder(); self.text_head.weight = _p(number_text_tokens, d); self.text_head.bias = _p(number_text_tokens, std=0)
        self.mel_head = _Holder(); self.mel_head.weight = _p(num_audio_tokens, d); self.mel_head.bias = _p(num_audio_tokens, std=0)
        # hyper-parameters hard-coded in the reference (gpt.py:179-188)
        self.conditioning_perceiver = PerceiverResampler(dim=d, depth=4, dim_context=80, num_latents=32, dim_head=64,
                                                         heads=8, ff_mult=4, use_flash_attn=False)
        self.engine = None
        self._prefix = None
        self.max_slots = 8
        self.recoveries = 0          # generations repeated after a hand-off time-out of a one-launch step (_recovering)
        self.last_ras_redraws = None # int32 [rows] redraws of the last generate() / get_generator() that used ras_window, else None

    # ------------------------------------------------------------------------------------------
    def dims(self):
        return dict(n_layer=self.layers, d_model=self.model_dim, n_head=self.heads,
                    num_audio_tokens=self.num_audio_tokens, number_text_tokens=self.number_text_tokens,
                    start_text_token=self.start_text_token, stop_text_token=self.stop_text_token,
                    start_audio_token=self.start_audio_token, stop_audio_token=self.stop_audio_token,
                    max_gen_mel_tokens=self.max_gen_mel_tokens, max_mel_pos=self.max_mel_tokens,
                    max_text_pos=self.max_text_tokens, max_prompt_tokens=self.max_prompt_tokens,
                    code_stride_len=self.code_stride_len,
                    max_seq=self.max_prompt_tokens + self.max_mel_tokens + self.max_text_tokens + 1)   # gpt.py:198

    def init_gpt_for_inference(self, kv_cache=True, use_deepspeed=False, max_slots=8, max_rows=4096, weight_dtype="fp32"):
        """reference gpt.py:197-218: here = create the HIP context and repack the weights into it.
        weight_dtype: "fp32" (reference numerics), "bf16" (bf16 weight storage), "bf16_kv" (+ bf16 KV cache), "bf16_act" (+ bf16
        activations across the hand-offs of the one-launch rows step: include/genvc_hip.h, weight_dtype 3) or "bf16_mfma" (+ the same
        rounding points and bf16 matrix cores on every other multi-row pass -- prefills, cached chunk prefills, the latent re-pass,
        verification rows, 17+ streams: weight_dtype 4; a second bf16 copy of the block matrices, 24 d^2 bytes per layer)."""
        if not kv_cache:
            raise NotImplementedError("the HIP path always uses the KV cache")
        if use_deepspeed:
            raise NotImplementedError("DeepSpeed kernel injection is replaced by libgenvc_hip")
        if self.engine is not None:
            self.engine.close()
        self.max_slots = max_slots
        self.engine = GptEngine(self.dims(), max_slots=max_slots, max_rows=max_rows, weight_dtype=weight_dtype)
        sd = {k: v for k, v in self.state_dict().items() if not k.startswith("conditioning_perceiver.")}
        self.engine.bind(sd)
        self.conditioning_perceiver.bind()
        return self

    def _need_engine(self):
        if self.engine is None:
            raise RuntimeError("call init_gpt_for_inference() first (reference inference/model_init.py:31)")

    def _recovering(self, n_slots, fn):
        """fn() -- a whole generation that has not handed anything to its caller yet -- with ONE retry after a hand-off time-out of a
        one-launch step (another context held CUs: include/genvc_hip.h, gvc_gpt_health).  The failed attempt's tokens and K/V rows are
        garbage; the library has already switched this context to the launch-per-phase paths, so the slots are reset and the work is
        repeated there.  Either the caller gets the tokens of a clean run or the error propagates: never the garbage
        (reference semantics: a call returns its tokens or fails, /root/reference/inference/inference_utils.py:135-217).  Other
        state errors (a full KV cache) are not recoverable by repeating and propagate at once."""
        try:
            return fn()
        except GenvcHipError as e:
            if not e.is_handoff_timeout:
                raise
            self.recoveries = getattr(self, "recoveries", 0) + 1
            torch.cuda.synchronize()
            dev = next(self.parameters()).device
            self.engine.reset(torch.arange(n_slots, device=dev, dtype=torch.int32))
            return fn()

    # ------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def get_style_emb(self, cond_input, return_latent=False, seq_lens=None, frames_major=None):
        """cond_input (b,80,s) or (b,1,80,s) -> (b, d, 32)   (reference gpt.py:351-373).  frames_major (extension): the same mel as
        (b,s,80), which the mel kernel writes alongside -- saves the permute(0, 2, 1).contiguous() copy in front of the Perceiver"""
        if return_latent:
            return cond_input.unsqueeze(1)
        if cond_input.ndim == 4:
            cond_input = cond_input.squeeze(1)
        x = frames_major if frames_major is not None else cond_input.permute(0, 2, 1).contiguous()
        mask = None
        if seq_lens is not None:              # gpt.py:362-367 (seq_lens in frames)
            mask = perceiver_key_mask(seq_lens, x.shape[1], self.conditioning_perceiver.cfg["num_latents"])
        return self.conditioning_perceiver(x, mask=mask).transpose(1, 2)

    @torch.inference_mode()
    def compute_embeddings(self, cond_latents, text_inputs):
        """reference gpt.py:572-592: stores the prefix embeddings, returns the fake ids (1 ... 1, start)."""
        self._need_engine()
        self._prefix = self.engine.prefix_embeddings(cond_latents.to(torch.float32).contiguous(),
                                                     text_inputs.to(torch.int32).contiguous())
        self._n_cond = int(cond_latents.shape[1])
        B, P, _ = self._prefix.shape
        ids = torch.full((B, P + 1), 1, dtype=torch.long, device=text_inputs.device)
        ids[:, -1] = self.start_audio_token
        return ids

    def _start(self, fake_inputs, kw, fan=1):
        """prefill + device-side loop state for the stored prefix.  fan = N > 1 (generate(num_return_sequences=N)): fake_inputs has N
        rows per item of the prefix, row b*N + j the j-th candidate of item b; item b is prefilled once, into slot b*N, and fanned out
        to the slots of its other candidates (engine.kv_fanout)"""
        _no_beams(kw, "streaming (get_generator)")
        _no_contrastive(kw, "streaming (get_generator)")
        B, n0 = fake_inputs.shape
        dev = fake_inputs.device
        max_new = kw.get("max_new_tokens") or self.max_gen_mel_tokens                     # gpt.py:606,618
        slots = torch.arange(B, device=dev, dtype=torch.int32)
        ids = torch.empty(B, n0 + max_new + 8, device=dev, dtype=torch.int32)
        ids[:, :n0] = fake_inputs.to(torch.int32)
        st = dict(B=B, slots=slots, ids=ids,
                  ids_len=torch.full((B,), n0, device=dev, dtype=torch.int32),
                  finished=torch.zeros(B, device=dev, dtype=torch.int32),
                  toks=torch.full((B, max_new), self.stop_audio_token, device=dev, dtype=torch.int32),
                  lats=torch.empty(B, max_new, self.model_dim, device=dev, dtype=torch.float32),
                  max_new=max_new, done=0, n0=n0)
        samp = dict(repetition_penalty=kw.get("repetition_penalty", 1.0), temperature=kw.get("temperature", 1.0),
                    top_p=kw.get("top_p", 1.0), top_k=kw.get("top_k", 0) if kw.get("do_sample", True) else 1)
        # green-list watermark (engine.WATERMARK_KWARGS): one call-wide entry; its table sits in a slot of the engine's
        # arena, held while this loop state lives.  Greedy search has no Temperature: the bias is added to the processed row as it is
        wm = _watermark(kw, self.num_audio_tokens)
        st["wm"] = None
        if wm is not None:
            st["wm"] = WatermarkTable([self.engine.watermark_entry(wm)], self.engine)
            if not kw.get("do_sample", True):
                samp["temperature"] = 1.0
        st["params"] = sample_params(samp, self.num_audio_tokens, self.stop_audio_token, kw.get("seed", 0))
        # length / repetition processors (HF kwargs, engine.PROC_KWARGS): the prompt is the fake ids
        st["proc"] = logits_processors(kw, n0, self.num_audio_tokens, sampling=kw.get("do_sample", True))
        # typical / epsilon / eta warpers (engine.WARP_KWARGS): with any on, the call carries them with its processors as one entry
        warp = logits_warpers(kw, sampling=kw.get("do_sample", True))
        st["warp"] = None if warp is None else WarperSets.one(st["proc"], warp, B)
        # sequence bias / bad words / forced EOS / renormalised scores (engine.BIAS_KWARGS): one call-wide struct, None when all are off
        st["bias"] = logits_bias(kw, n0, max_new, self.num_audio_tokens, self.stop_audio_token)
        # repetition-aware sampling (engine.RAS_KWARGS): one call-wide entry counting from the fake ids, and the rows' redraw counters
        st["ras"] = None
        if _ras_on(kw):
            st["ras"] = RasTable([logits_ras(kw, n0)], torch.zeros(B, device=dev, dtype=torch.int32))
        self.last_ras_redraws = None if st["ras"] is None else st["ras"].redraws
        # presence / frequency / windowed repetition penalties (engine.PENALTY_KWARGS): one call-wide entry counting from the fake ids
        pen = logits_penalties(kw, n0)
        st["pen"] = None if pen is None else PenaltyTable([pen])
        # `cached_cond_rows` (extension): the leading rows of the prefix -- the conditioning latents, identical for every
        # segment of an utterance -- are still in the KV cache from the previous segment's prefill of these slots
        if fan > 1:
            src = slots[::fan].contiguous()
            self.engine.prefill(src, self._prefix, want_outputs=False, n_cached=int(kw.get("cached_cond_rows", 0)))
            self.engine.kv_fanout(src.repeat_interleave(fan - 1), slots.view(-1, fan)[:, 1:].reshape(-1).contiguous())
            return st
        self.engine.prefill(slots, self._prefix, want_outputs=False, n_cached=int(kw.get("cached_cond_rows", 0)))
        return st

    def _advance(self, st, n):
        """n graph-replayed (sample, decode) steps; returns True when every row has emitted the stop token"""
        n = min(n, st["max_new"] - st["done"])
        if n > 0:
            # the cache holds n0 positions after the prefill and one more per step: the library picks its decode kernels for the
            # context length this call reaches (not for the 602-token cap the ids rows are sized for); under guidance the longer of the
            # two contexts bounds the keys.  One call whatever the loop state holds (processors, warpers, sequence bias, the buffers of
            # output_scores / output_logits, unconditional slots): generate_call picks the entry, on the engine or a stand-in for it
            _generate_call(self.engine, st["slots"], st["ids"], st["ids_len"], st["finished"], st["params"], st["done"], n, st["toks"],
                           st["lats"], max_keys=max(st["n0"], st.get("n0_uncond", 0)) + st["done"] + n, proc=st["proc"],
                           sets=st["warp"], bias=st.get("bias"), uncond_slots=st.get("uncond_slots"),
                           scale=st.get("guidance_scale", 1.0), scores_out=st.get("scores"), logits_out=st.get("raw_logits"),
                           do_sample=st.get("do_sample", True), **({} if st.get("ras") is None else {"ras": st["ras"]}),
                           **({} if st.get("pen") is None else {"pen": st["pen"]}),
                           **({} if st.get("wm") is None else {"wm": st["wm"]}))
            st["done"] += n
        end = bool(st["finished"].all().item()) or st["done"] >= st["max_new"]
        self.engine.health()          # (the .item() above synchronised: a hand-off timeout of these steps surfaces here, not a call later)
        return end

    def _step_outputs(self, st, kw):
        """the per-step buffers of a call with output_scores / output_logits, allocated only when asked for ([rows, max_new, V] fp32
        each) and filled by _advance"""
        _, want_scores, want_logits = _output_kwargs(kw)
        shape = (st["B"], st["max_new"], self.num_audio_tokens)
        dev = st["ids"].device
        st["scores"] = torch.empty(shape, device=dev, dtype=torch.float32) if want_scores else None
        st["raw_logits"] = torch.empty(shape, device=dev, dtype=torch.float32) if want_logits else None
        st["do_sample"] = bool(kw.get("do_sample", True))

    def _result(self, ids, kw, st=None, n=0, beams=False):
        """what generate() returns: the tokens, or with return_dict_in_generate=True a GenerateOutput around them"""
        if not _output_kwargs(kw)[0]:
            return ids

        def steps(buf):
            return None if buf is None else tuple(buf[:, t] for t in range(n))
        out = GenerateOutput(sequences=ids, scores=steps(st.get("scores")) if st else None,
                             logits=steps(st.get("raw_logits")) if st else None, latents=self.last_latents,
                             sequences_scores=self.last_beam_scores if beams else None)
        if st and any(_trace_kwargs(kw)):
            out["attentions"], out["hidden_states"] = self._trace_steps(st, ids, kw)
        if st and st.get("ras") is not None:          # (only in the result of a call that used RAS)
            out["ras_redraws"] = st["ras"].redraws
        return out

    def _trace_ready(self, kw, rows):
        """before a call with output_attentions / output_hidden_states spends its steps: the context's numerics and the smallest size
        the attentions can have (the exact size is checked once the tokens are final)"""
        at, hs = _trace_kwargs(kw)
        if not (at or hs):
            return
        wd = getattr(self.engine, "weight_dtype", "fp32")
        if wd != "fp32":
            raise NotImplementedError(f"output_attentions / output_hidden_states with weight_dtype=\"{wd}\" are not implemented: the "
                                      "trace pass is a reference-numerics pass (init_gpt_for_inference(weight_dtype=\"fp32\"))")
        if at:
            _trace_bytes_check(self.layers, rows, self.heads, int(self._prefix.shape[1]) + 1, int(kw.get("max_trace_bytes", MAX_TRACE_BYTES)))

    def _trace_steps(self, st, ids, kw):
        """the trace pass of a finished sampler call (engine.trace; include/genvc_hip.h: gvc_gpt_trace) on the call's slots, from its
        prefix embeddings and its final ids [rows, n], cut into HF's per-step views -> (attentions, hidden_states)"""
        at, hs = _trace_kwargs(kw)
        rows, n = int(ids.shape[0]), int(ids.shape[1])
        prefix = self._prefix
        if int(prefix.shape[0]) != rows:                     # num_return_sequences: row b*N + j is candidate j of item b
            prefix = prefix.repeat_interleave(rows // int(prefix.shape[0]), 0)
        P = int(prefix.shape[1])
        if at:
            _trace_bytes_check(self.layers, rows, self.heads, P + n, int(kw.get("max_trace_bytes", MAX_TRACE_BYTES)))
        probs, hidden, _ = self.engine.trace(st["slots"], prefix, ids.to(torch.int32), self._code_lengths(ids), self._n_cond,
                                             output_attentions=at, output_hidden_states=hs, alignment=False)
        return _step_views(probs, hidden, P, n)

    def _code_lengths(self, toks):
        """generated length per row, its stop code counted; n for a row that never stopped"""
        is_stop = toks == self.stop_audio_token
        first = is_stop.long().argmax(1) + 1
        return torch.where(is_stop.any(1), first, torch.full_like(first, toks.shape[1])).to("cpu", torch.int32)

    @torch.inference_mode()
    def trace(self, cond_latents, text_inputs, codes, code_lengths=None, output_attentions=True, output_hidden_states=False,
              alignment_layers=None, max_trace_bytes=MAX_TRACE_BYTES):
        """Attention weights, hidden states and the content alignment of given acoustic codes [B, n] under the prompt (cond_latents,
        text_inputs): one teacher-forced pass over [prefix | start, codes[:, :n-1]] (include/genvc_hip.h: gvc_gpt_trace; DESIGN.md
        4.23), row P + i the query of the step that produced code i.  code_lengths [B]: each row's generated length, its stop code
        counted (default: up to and including the row's first stop token, else n); steps at or past it are zeros -- HF's generate
        returns the attention of the pad inputs it fed such rows, which means nothing.
        -> GenerateOutput: sequences = codes; attentions fp32 [L, B, H, T, T] (T = P + n; zero above the diagonal) or None;
        hidden_states fp32 [L+1, B, T, D] (embeddings, each layer's output, ln_f of the last) or None; alignment fp32 [B, n, Tc]: the
        mean over the heads of `alignment_layers` (indices, negative from the end; default all) of the weight step i puts on the Tc
        content codes.  Of the prefix rows [conditioning (32) | text start | content codes | text stop] (compute_embeddings, reference
        gpt.py:572-592) only the content codes count: a row of `alignment` sums to at most 1, the rest of the mass sits on the
        conditioning rows, the text start / stop rows and the acoustic codes in front.  fp32 contexts only."""
        self._need_engine()
        wd = getattr(self.engine, "weight_dtype", "fp32")
        if wd != "fp32":
            raise NotImplementedError(f"GPT.trace with weight_dtype=\"{wd}\" is not implemented: the trace pass is a reference-numerics "
                                      "pass (init_gpt_for_inference(weight_dtype=\"fp32\"))")
        prefix = self.engine.prefix_embeddings(cond_latents.to(torch.float32).contiguous(), text_inputs.to(torch.int32).contiguous())
        B, P, _ = prefix.shape
        n = int(codes.shape[1])
        if output_attentions:
            _trace_bytes_check(self.layers, B, self.heads, P + n, int(max_trace_bytes))
        lengths = self._code_lengths(codes) if code_lengths is None else torch.as_tensor(code_lengths).to("cpu", torch.int32)
        slots = torch.arange(B, device=prefix.device, dtype=torch.int32)
        probs, hidden, align = self.engine.trace(slots, prefix, codes.to(device=prefix.device, dtype=torch.int32), lengths,
                                                 int(cond_latents.shape[1]), output_attentions=output_attentions,
                                                 output_hidden_states=output_hidden_states, alignment=True, alignment_layers=alignment_layers)
        return GenerateOutput(sequences=codes, scores=None, logits=None, latents=None, sequences_scores=None, attentions=probs,
                              hidden_states=hidden, alignment=align)

    @torch.inference_mode()
    def compute_transition_scores(self, sequences, scores, normalize_logits=False):
        """transformers' GenerationMixin.compute_transition_scores without beams, on the device (include/genvc_hip.h:
        gvc_transition_scores): sequences int64 [rows, n] and scores (a GenerateOutput's `scores` or `logits`: n rows of [rows, V]) ->
        fp32 [rows, n], the score of every generated token, behind a log_softmax over the vocabulary with normalize_logits=True.
        Longer sequences are read from their last n columns, as HF cuts the prompt away."""
        self._need_engine()
        scores = tuple(scores)
        n = len(scores)
        V = self.num_audio_tokens
        if n == 0:
            return torch.empty(int(sequences.shape[0]), 0, device=sequences.device, dtype=torch.float32)
        s0 = scores[0]
        # the views generate() hands out share one [rows, max_new, V] tensor: read in place
        if all(s.shape == s0.shape and s.stride() == s0.stride() and s.data_ptr() == s0.data_ptr() + 4 * V * t
               for t, s in enumerate(scores)) and s0.ndim == 2 and s0.stride(1) == 1 and (s0.shape[0] == 1 or s0.stride(0) >= n * V):
            stacked = torch.as_strided(s0, (s0.shape[0], n, V), (s0.stride(0) if s0.shape[0] > 1 else n * V, V, 1))
        else:
            stacked = torch.stack([s.to(torch.float32) for s in scores], 1).contiguous()
        toks = sequences[:, -n:].to(device=stacked.device, dtype=torch.int32).contiguous()
        return self.engine.transition_scores(stacked, toks, normalize=normalize_logits)

    @torch.inference_mode()
    def generate(self, cond_latents, text_inputs, **generate_kwargs):
        """reference gpt.py:594-609 -> int64 [B, n_generated]; finished rows are padded with the stop token.
        `group` (extra kwarg) = decode steps per host check of the finished flags.
        num_beams = K > 1 with do_sample=False: deterministic beam search on the device (_generate_beams).
        top_k = K > 1 with do_sample=False and penalty_alpha > 0: contrastive search on the device (_generate_contrastive), before
        num_beams as in transformers 4.33.
        num_return_sequences = N > 1 when sampling: int64 [B*N, n], row b*N + j the j-th candidate of item b, as HF's input expansion
        (repeat_interleave(N)) orders them -- and draws them: the sampler keys a draw by (seed, step, row).  Item b is prefilled once
        and its KV slot fanned out to its candidates' slots (needs B*N <= the context's KV slots, ValueError otherwise); the B*N rows
        then decode together.  `last_latents` is [B*N, n, d]; `last_sequence_logprobs` / `last_sequence_lengths` hold
        sequence_logprobs() of the candidates (an extension: a score to rank them by).  Greedy decoding with N > 1 raises ValueError.
        guidance_scale = s != 1 with negative_cond_latents: classifier-free guidance on the device (_generate_guided), checked before
        the other modes; None or 1 is exactly the call without it (negative_* are then ignored, as HF ignores negative_prompt_ids).
        return_dict_in_generate=True: a GenerateOutput (sequences = the tensor above, latents, sequences_scores for beams) instead
        of the tensor; with it output_scores=True / output_logits=True add `scores` / `logits`, tuples of n fp32 [rows, V] rows, as
        transformers' _sample fills them -- on the sampler paths (greedy, sampling, every processor and warper,
        num_return_sequences, guidance_scale); with beams, beam groups or contrastive search they raise NotImplementedError.  The
        tokens are those of the call without the kwargs, bit for bit.  Without return_dict_in_generate the other two are ignored.
        output_attentions=True / output_hidden_states=True (with return_dict_in_generate, else ignored as HF ignores them): `attentions`
        / `hidden_states` in HF's per-step form (GenerateOutput), from one trace pass over the final ids after the
        loop (gvc_gpt_trace) on the same sampler paths -- under guidance the conditional rows, which are what HF's model call sees.
        Steps at or past a row's end are zeros (HF returns the attention of its pad inputs there).  Beams, beam groups, contrastive
        search, assisted and prompt-lookup decoding raise NotImplementedError, as does a context whose weight_dtype is not "fp32";
        attentions above max_trace_bytes (default 2 GiB) raise ValueError.  The tokens are those of the call without the kwargs.
        sequence_bias / bad_words_ids / forced_eos_token_id / renormalize_logits (engine.logits_bias; include/genvc_hip.h:
        gvc_logits_bias): transformers' SequenceBias, NoBadWords, ForcedEOSToken and LogitNormalization processors at
        their places in HF's list, on the same sampler paths (under guidance on the guided row).  sequence_bias ids may be 0 in both of
        its forms (HF's list form refuses 0); forced_eos_token_id must be the stop token and fires at the step that writes token
        max_new_tokens - 1; renormalize_logits makes the stored `scores` log-probabilities and leaves the tokens those of the call
        without it, bit for bit (no effect without output_scores).  forced_bos_token_id is accepted and does nothing: HF's processor
        fires at cur_len == 1, and no prompt of this model is that short.  Beams, beam groups and contrastive search raise
        NotImplementedError for them, as the grouped, rolling, session and streaming paths do.
        ras_window = K (1..64) [, ras_threshold = t in (0, 1], default 0.1]: repetition-aware sampling (engine.logits_ras;
        include/genvc_hip.h: gvc_logits_ras) on the same sampler paths: a step whose token fills max(1, ceil(t K)) of
        the row's last K generated tokens draws again from the distribution ahead of top-k / top-p / the warpers.  top_k=1 with it is
        greedy decoding with an escape; do_sample=False raises ValueError pointing there.  `last_ras_redraws` (and `ras_redraws` of a
        GenerateOutput) count each row's redraws; scores and logits stay those of the first draw.  None or 0 is exactly the call
        without it.  Beams, beam groups, contrastive search, assisted and prompt-lookup decoding raise NotImplementedError.
        presence_penalty = p, frequency_penalty = f (each in [-2, 2]), penalty_window = W (engine.logits_penalties;
        include/genvc_hip.h: gvc_logits_penalties) on the same sampler paths, greedy search included: an id that
        occurs c > 0 times among the row's last W generated tokens (all of them without a window; the fake prompt ids never count)
        loses f * c + p, directly behind the repetition penalty; with W > 0 the repetition penalty too covers only those ids
        (repetition_penalty=2.0, penalty_window=16 is a windowed repetition penalty).  `scores` carry them, `logits` stay raw.
        Each None or 0 is exactly the call without it.  Beams, beam groups, contrastive search, assisted and prompt-lookup
        decoding raise NotImplementedError.
        watermarking_config = a dict with transformers' keys (greenlist_ratio 0.25, bias 2.0, hashing_key 15485863, seeding_scheme
        "lefthash" | "selfhash", context_width 1) or an object with to_dict() such as transformers' WatermarkingConfig
        (engine.watermark_settings; include/genvc_hip.h: gvc_logits_watermark): the green-list watermark of
        Kirchenbauer et al. with transformers' semantics -- behind every processor and warper, ahead of renormalize_logits, the green
        list of a step chosen by the previous code (at the first step the fake prompt's last id).  key -> green lists is defined by
        the CPU torch.Generator: engine.WatermarkDetector / GenVCModel.detect_watermark, or transformers' detector built with
        device="cpu", find the mark.  `scores` carry the bias, `logits` stay raw.  A green stop code is biased like any other, so a
        marked call can end earlier or later than the unmarked one.  Greedy search (do_sample=False, lefthash) takes the argmax of
        the biased row; do_sample=True with top_k=1 raises ValueError (nothing could be marked), selfhash with greedy search or
        typical_p, ras_window, beams, beam groups, contrastive search, assisted and prompt-lookup decoding raise
        NotImplementedError.  None is exactly the call without it.  generate_groups / generate_rolling take it call-wide and per
        group / job (group_kwargs / job_kwargs: two keys in one call), StreamSessions per session, on sampled rows.
        assistant_model = another initialised GPT: assisted (speculative) greedy decoding (_generate_assisted), checked
        before every other mode; the tokens are those of the call without it.  None is exactly that call.  With
        speculative_sampling=True a sampled call is served too (speculative sampling: same distribution per token, other tokens than
        the plain call with that seed; _generate_assisted).
        prompt_lookup_num_tokens = k (1..15) [, max_matching_ngram_size = N (1..8, default 2)]: assisted decoding without a draft
        model (_generate_assisted) -- the drafts of a round are the k ids that followed the earliest earlier
        occurrence of the row's last up-to-N generated ids.  Greedy (the tokens of the call without it), or sampled with
        speculative_sampling=True.  With assistant_model, or max_matching_ngram_size alone: ValueError."""
        _num_return(generate_kwargs)
        if _lookup(generate_kwargs) or generate_kwargs.get("assistant_model") is not None:
            _no_ras(generate_kwargs, _LOOKUP_MODE if _lookup(generate_kwargs) else "assisted decoding (assistant_model)")
            _no_penalties(generate_kwargs, _LOOKUP_MODE if _lookup(generate_kwargs) else "assisted decoding (assistant_model)")
            _no_watermark(generate_kwargs, _LOOKUP_MODE if _lookup(generate_kwargs) else "assisted decoding (assistant_model)",
                          self.num_audio_tokens)
            return self._generate_assisted(cond_latents, text_inputs, generate_kwargs)
        if ras_counts(generate_kwargs) is not None:
            if _contrastive_mode(generate_kwargs) is not None:
                _no_ras(generate_kwargs, f"contrastive search (penalty_alpha={generate_kwargs.get('penalty_alpha')})")
            if _grouped(generate_kwargs):
                _no_ras(generate_kwargs, "beam groups (num_beam_groups / diversity_penalty)")
            if int(generate_kwargs.get("num_beams", 1) or 1) > 1:
                _no_ras(generate_kwargs, f"beam search (num_beams={generate_kwargs.get('num_beams')})")
            _ras_on(generate_kwargs)          # (do_sample=False: ValueError)
        if penalty_settings(generate_kwargs) is not None:
            if _contrastive_mode(generate_kwargs) is not None:
                _no_penalties(generate_kwargs, f"contrastive search (penalty_alpha={generate_kwargs.get('penalty_alpha')})")
            if _grouped(generate_kwargs):
                _no_penalties(generate_kwargs, "beam groups (num_beam_groups / diversity_penalty)")
            if int(generate_kwargs.get("num_beams", 1) or 1) > 1:
                _no_penalties(generate_kwargs, f"beam search (num_beams={generate_kwargs.get('num_beams')})")
        if watermark_settings(generate_kwargs, self.num_audio_tokens) is not None:
            if _contrastive_mode(generate_kwargs) is not None:
                _no_watermark(generate_kwargs, f"contrastive search (penalty_alpha={generate_kwargs.get('penalty_alpha')})",
                              self.num_audio_tokens)
            if _grouped(generate_kwargs):
                _no_watermark(generate_kwargs, "beam groups (num_beam_groups / diversity_penalty)", self.num_audio_tokens)
            if int(generate_kwargs.get("num_beams", 1) or 1) > 1:
                _no_watermark(generate_kwargs, f"beam search (num_beams={generate_kwargs.get('num_beams')})", self.num_audio_tokens)
            _watermark(generate_kwargs, self.num_audio_tokens)          # (the refused combinations raise before any work is done)
        scale = _guidance_scale(generate_kwargs)
        if scale is not None:
            return self._generate_guided(cond_latents, text_inputs, scale, generate_kwargs)
        if _contrastive_kwargs(generate_kwargs) is not None:
            _no_bias(generate_kwargs, f"contrastive search (penalty_alpha={generate_kwargs.get('penalty_alpha')})")
            _no_step_outputs(generate_kwargs, f"contrastive search (penalty_alpha={generate_kwargs.get('penalty_alpha')})")
            _no_trace(generate_kwargs, f"contrastive search (penalty_alpha={generate_kwargs.get('penalty_alpha')})")
            return self._result(self._generate_contrastive(cond_latents, text_inputs, generate_kwargs), generate_kwargs)
        if int(generate_kwargs.get("num_beams", 1) or 1) > 1 or _grouped(generate_kwargs):
            _no_bias(generate_kwargs, "beam groups (num_beam_groups / diversity_penalty)" if _grouped(generate_kwargs)
                     else f"beam search (num_beams={generate_kwargs.get('num_beams')})")
            _no_step_outputs(generate_kwargs, "beam groups (num_beam_groups / diversity_penalty)" if _grouped(generate_kwargs)
                             else f"beam search (num_beams={generate_kwargs.get('num_beams')})")
            _no_trace(generate_kwargs, "beam groups (num_beam_groups / diversity_penalty)" if _grouped(generate_kwargs)
                      else f"beam search (num_beams={generate_kwargs.get('num_beams')})")
            return self._result(self._generate_beams(cond_latents, text_inputs, generate_kwargs), generate_kwargs, beams=True)
        N = _sample_return_kwargs(generate_kwargs, int(text_inputs.shape[0]), self.max_slots)
        fake = self.compute_embeddings(cond_latents, text_inputs)
        if N > 1:
            fake = fake.repeat_interleave(N, 0)
        self._trace_ready(generate_kwargs, int(fake.shape[0]))
        group = generate_kwargs.pop("group", 16)

        attempt = []

        def run():
            # (a retry after a hand-off time-out prefills in full: the reset slots have lost any cached conditioning rows)
            st = self._start(fake, dict(generate_kwargs, cached_cond_rows=0) if attempt else generate_kwargs, fan=N)
            attempt.append(1)
            self._step_outputs(st, generate_kwargs)
            while not self._advance(st, group):
                pass
            return st
        return self._finish(self._recovering(int(fake.shape[0]), run), generate_kwargs, N)

    def _finish(self, st, kw, N=1):
        """what a finished sampler loop returns: the reference loop stops at the step where the last row emits 1025"""
        toks = st["toks"][:, :st["done"]].long()
        n = self._stop_len(toks)
        self.last_latents = st["lats"][:, :n]
        self.last_sequence_logprobs = self.last_sequence_lengths = None
        if N > 1:
            self.last_sequence_logprobs, self.last_sequence_lengths = self.sequence_logprobs(toks[:, :n], self.last_latents)
        if st.get("wm") is not None:
            st["wm"].release()          # (the loop has ended: its table's slot is free for others, whatever still refers to st)
        return self._result(toks[:, :n], kw, st, n)

    def _generate_guided(self, cond_latents, text_inputs, scale, generate_kwargs):
        """HF generate(guidance_scale=s, negative_prompt_ids=...) semantics on a prefix-embedded model (include/genvc_hip.h:
        gvc_gpt_generate_cfg; transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor): item b decodes under two prompts, the
        conditional (cond_latents[b], text_inputs[b]) in KV slot b and the unconditional (negative_cond_latents[b],
        negative_text_inputs[b], default text_inputs[b]) in slot B + b; a leading dimension of 1 broadcasts, and the negative code
        length may differ.  Every step samples item b from s * (lsm(cond) - lsm(uncond)) + lsm(uncond) -- the guidance processor comes
        first in HF's list, so the repetition penalty, the processors, temperature / top-k / top-p and the warpers run on it with the
        conditional row's ids -- and feeds the token to both slots.  The unconditional prompt always prefills in full.  Needs 2B <= the
        context's KV slots.  Returns int64 [B, n] as generate(); `last_latents` are the conditional rows' latents.  Beams, beam
        groups, contrastive search and num_return_sequences > 1 raise NotImplementedError under guidance."""
        kw = dict(generate_kwargs)
        if _contrastive_mode(kw) is not None:
            raise NotImplementedError(f"guidance_scale={scale} with contrastive search (penalty_alpha={kw.get('penalty_alpha')}) is not "
                                      "implemented")
        if _grouped(kw):
            raise NotImplementedError(f"guidance_scale={scale} with beam groups (num_beam_groups={kw.get('num_beam_groups')}, "
                                      f"diversity_penalty={kw.get('diversity_penalty')}) is not implemented")
        if int(kw.get("num_beams", 1) or 1) > 1:
            raise NotImplementedError(f"guidance_scale={scale} with beam search (num_beams={kw.get('num_beams')}) is not implemented")
        if _num_return(kw) > 1:
            raise NotImplementedError(f"guidance_scale={scale} with num_return_sequences={kw.get('num_return_sequences')} is not "
                                      "implemented")
        neg = kw.pop("negative_cond_latents", None)
        neg_text = kw.pop("negative_text_inputs", None)
        if neg is None:
            raise ValueError(f"guidance_scale={scale} needs negative_cond_latents: HF's default unconditional prompt is the bare last "
                             "token, which means nothing to a model whose prompt is an embedded prefix")
        B = int(text_inputs.shape[0])
        if neg.ndim != 3 or int(neg.shape[0]) not in (1, B) or int(neg.shape[2]) != self.model_dim:
            raise ValueError(f"negative_cond_latents must be [1 or {B}, n, {self.model_dim}], not {list(neg.shape)}")
        if neg_text is None:
            neg_text = text_inputs
        if neg_text.ndim != 2 or int(neg_text.shape[0]) not in (1, B):
            raise ValueError(f"negative_text_inputs must be [1 or {B}, n_codes], not {list(neg_text.shape)}")
        if 2 * B > self.max_slots:
            raise ValueError(f"classifier-free guidance over {B} items needs {2 * B} KV slots; the context has {self.max_slots} "
                             "(init_gpt_for_inference(max_slots=...))")
        self._need_engine()
        group = kw.pop("group", 16)
        fake = self.compute_embeddings(cond_latents, text_inputs)
        dev = fake.device
        neg = neg.to(device=dev, dtype=torch.float32).expand(B, -1, -1).contiguous()
        neg_text = neg_text.to(device=dev, dtype=torch.int32).expand(B, -1).contiguous()
        uprefix = self.engine.prefix_embeddings(neg, neg_text)
        self._trace_ready(kw, B)
        attempt = []

        def run():
            st = self._start(fake, dict(kw, cached_cond_rows=0) if attempt else kw)
            attempt.append(1)
            st["uncond_slots"] = torch.arange(B, 2 * B, device=dev, dtype=torch.int32)
            st["guidance_scale"] = scale
            st["n0_uncond"] = int(uprefix.shape[1]) + 1
            self.engine.prefill(st["uncond_slots"], uprefix, want_outputs=False)      # (always in full: no cached rows on these slots)
            self._step_outputs(st, kw)
            while not self._advance(st, group):
                pass
            return st
        return self._finish(self._recovering(2 * B, run), kw)

    def _generate_assisted(self, cond_latents, text_inputs, generate_kwargs):
        """HF generate(assistant_model=draft, do_sample=False) semantics on the device (include/genvc_hip.h: gvc_gpt_generate_assisted):
        `assistant_model` is a GPT after init_gpt_for_inference with this model's num_audio_tokens, start and stop audio tokens; it
        builds its own prefix from `assistant_cond_latents` (required when its model_dim differs, else cond_latents is reused) and
        the same text_inputs, and prefills its own KV slots.  Every round the assistant drafts k = num_assistant_tokens (1..15,
        default 5, the choice of profiles/assisted_decoding.md) tokens greedily, this model scores [pending token, d_1..d_k] in one
        multi-row pass, the device accepts the longest agreeing prefix plus one token of this model per row, and both caches roll
        back; near the end of the position tables a call drafts fewer tokens.  Greedy (do_sample=False or top_k=1), with
        repetition_penalty, temperature and the processor kwargs (engine.PROC_KWARGS) on both models; every other mode raises
        NotImplementedError.
        speculative_sampling=True (opt-in; without it a sampled call is refused as before) with do_sample (default True) and
        top_k != 1: speculative sampling (Leviathan et al.; include/genvc_hip.h: gvc_gpt_generate_assisted_sample).
        The draft SAMPLES its k tokens with the call's top_k / top_p / temperature / repetition_penalty / processors (min_p included),
        draft d is accepted with probability min(1, p(d) / q(d)) under the two models' warped rows, and the token behind the accepted
        prefix is drawn from max(p - q, 0) (from p behind k accepted drafts).  Each emitted token is distributed as a plain sampled
        token of this model under the same warpers; the tokens are NOT those of the plain call with the same `seed` -- the uniforms
        are keyed by (seed, position in the generation, 3 * row + {0: draft, 1: accept, 2: residual}), so they do not depend on
        `group` either.  do_sample=False or top_k=1 with the kwarg is the greedy mode above.
        prompt_lookup_num_tokens=k [, max_matching_ngram_size=N] instead of assistant_model (HF's PromptLookupCandidateGenerator;
        include/genvc_hip.h: gvc_gpt_generate_lookup): no draft model -- a round's drafts are the up to k ids that
        followed the earliest earlier occurrence of the row's last n <= N GENERATED ids, the longest n with a hit; the prompt's
        placeholder ids are never searched.  A row without a hit still pays the round's (k + 1)-row pass and emits one token.  Same
        modes, refusals, returns and stats; sampled, the draft rows are one-hot (accept d iff u_acc <= p(d)).  The host reads the finished flags once per max(1, group // (k + 1)) rounds.  Token 0 of a row comes from
        the prefill's logits (the opening step: no round is counted for it), so a row of n tokens whose drafts were all accepted ran
        ceil((n - 1) / (k + 1)) rounds.  Returns what the call without the assistant returns (tokens bit for bit; `last_latents`
        from the verification rows) and sets `last_assist_stats`: dict(rounds, drafted, accepted), int64 [B] each."""
        kw = dict(generate_kwargs)
        asst = kw.pop("assistant_model", None)
        acond = kw.pop("assistant_cond_latents", None)
        B = int(text_inputs.shape[0])
        lookup = asst is None          # (generate() sends a call here for an assistant or for prompt_lookup_num_tokens, never both)
        if lookup:
            k, ngram = _assisted_kwargs(kw, B, lookup=True)
        else:
            k = _assisted_kwargs(kw, B)
        spec = _speculative(kw)
        for name in ASSIST_KWARGS[1:3] + ASSIST_KWARGS[4:] + LOOKUP_KWARGS:
            kw.pop(name, None)
        mode = _LOOKUP_MODE if lookup else "assisted decoding (assistant_model)"
        if not lookup:
            if not isinstance(asst, GPT) or asst is self:
                raise ValueError(f"{mode}: assistant_model must be another GPT, not {type(asst).__name__ if asst is not self else 'the target itself'}")
            if asst.engine is None:
                raise ValueError(f"{mode}: the assistant is not initialised (call its init_gpt_for_inference() first)")
            for name in ("num_audio_tokens", "start_audio_token", "stop_audio_token"):
                if getattr(asst, name) != getattr(self, name):
                    raise ValueError(f"{mode}: the assistant's {name} is {getattr(asst, name)}, the target's {getattr(self, name)}")
            if acond is None:
                if asst.model_dim != self.model_dim:
                    raise ValueError(f"{mode}: assistant_cond_latents is required: the assistant's model_dim {asst.model_dim} differs "
                                     f"from the target's {self.model_dim}")
                acond = cond_latents
            if B > self.max_slots or B > asst.max_slots:
                raise ValueError(f"{mode}: {B} items need {B} KV slots in both contexts (target {self.max_slots}, assistant {asst.max_slots})")
        elif B > self.max_slots:
            raise ValueError(f"{mode}: {B} items need {B} KV slots (the context has {self.max_slots})")
        self._need_engine()
        group = int(kw.pop("group", 16))
        fake = self.compute_embeddings(cond_latents, text_inputs)
        n0 = int(fake.shape[1])
        a_n0 = n0 if lookup else int(asst.compute_embeddings(acond, text_inputs).shape[1])
        dev = fake.device
        max_new = int(kw.get("max_new_tokens") or self.max_gen_mel_tokens)
        if lookup and max_new + MAX_ASSISTANT_TOKENS + 1 > MAX_LOOKUP_HISTORY:
            raise ValueError(f"{mode}: max_new_tokens={max_new} is above the {MAX_LOOKUP_HISTORY - MAX_ASSISTANT_TOKENS - 1} generated "
                             "ids a lookup searches")

        # drafts that fit the position tables of both contexts (of this one, for a lookup) when the furthest live row has emitted ub
        # tokens: a round appends k + 1 rows at cache length n0 + ub - 1 and mel position ub, and both must end below the last table entry
        def fit(ub):
            f = []
            for m, p0 in ((self, n0),) if lookup else ((self, n0), (asst, a_n0)):
                f += [m.engine.dims["max_mel_pos"] - 2 - ub, m.engine.dims["max_seq"] - 2 - p0 - ub]
            return min(f)
        if max_new > 1 and fit(max_new - 1) < 1:
            raise ValueError(f"{mode}: max_new_tokens={max_new} leaves no room for a draft in the position tables; lower it")
        samp = dict(repetition_penalty=kw.get("repetition_penalty", 1.0), temperature=kw.get("temperature", 1.0),
                    top_p=kw.get("top_p", 1.0) if spec else 1.0, top_k=kw.get("top_k", 0) if spec else 1)
        if spec and not int(samp["top_k"]) <= self.num_audio_tokens:
            raise ValueError(f"{mode}: top_k={samp['top_k']} is above the vocabulary ({self.num_audio_tokens})")
        if spec and not float(samp["temperature"]) > 0.0:
            raise ValueError(f"{mode}: temperature={samp['temperature']} must be > 0")
        params = sample_params(samp, self.num_audio_tokens, self.stop_audio_token, kw.get("seed", 0))
        proc = logits_processors(kw, n0, self.num_audio_tokens, sampling=spec)
        per_check = max(1, group // (k + 1))
        more = dict(sampling=True) if spec else {}          # (the greedy mode makes exactly the call it made before)

        def run():
            slots = torch.arange(B, device=dev, dtype=torch.int32)
            self.engine.prefill(slots, self._prefix, want_outputs=False)
            if not lookup:
                asst.engine.prefill(slots, asst._prefix, want_outputs=False)
            st = AssistedState(fake, k, max_new, self.stop_audio_token, self.num_audio_tokens, self.model_dim)
            ub = 1          # tokens the furthest live row can have emitted (the opening step emits one)
            while True:
                # the rounds of one call draft the same count: as many rounds as that count fits (fit() only shrinks as rows advance)
                kc = min(k, fit(ub)) if max_new > 1 else 1
                n, u, reach = 0, ub, ub
                while max_new > 1 and n < per_check and min(k, fit(u)) >= kc:
                    reach = u + kc          # cached positions behind the prompt at the end of this round's verification
                    n, u = n + 1, min(max_new - 1, u + kc + 1)
                if lookup:
                    self.engine.generate_lookup(slots, st, params, n, n0 + reach, ngram, proc=proc, k=kc, **more)
                else:
                    self.engine.generate_assisted(asst.engine, slots, slots, st, params, n, n0 + reach, a_n0 + reach, proc=proc, k=kc, **more)
                ub = u
                end = bool(st.finished.all().item())
                self.engine.health()          # (the .item() above synchronised)
                if not lookup:
                    asst.engine.health()
                if end:
                    return st
        try:
            st = run()
        except GenvcHipError as e:
            if not e.is_handoff_timeout:
                raise
            # a hand-off time-out in either context (_recovering): both have switched paths where needed; reset and repeat in full
            self.recoveries = getattr(self, "recoveries", 0) + 1
            torch.cuda.synchronize()
            slots = torch.arange(B, device=dev, dtype=torch.int32)
            self.engine.reset(slots)
            if not lookup:
                asst.engine.reset(slots)
            st = run()
        toks = st.toks.long()
        n = self._stop_len(toks)
        self.last_latents = st.lats[:, :n]
        self.last_sequence_logprobs = self.last_sequence_lengths = None
        self.last_assist_stats = st.stats()
        return self._result(toks[:, :n], kw)

    @torch.inference_mode()
    def sequence_logprobs(self, tokens, latents):
        """Extension (the reference has no such score): tokens [R, n] and the generation loop's latents [R, n, d] (`last_latents`) ->
        (logprob [R] float64, length [R] int64), logprob[r] = sum over t < length[r] of log_softmax(mel_head(latents[r, t]))[tokens[r, t]],
        length[r] up to and including row r's first stop token (n without one).  The loop's latents are final_norm(ln_f(h)), so mel_head of
        them is the logits row each token was chosen from: this is the RAW model distribution -- no repetition penalty, logits
        processor or warper, whatever the call that produced the tokens used.  On the device (include/genvc_hip.h:
        gvc_gpt_sequence_logprobs)."""
        self._need_engine()
        n = int(latents.shape[1])
        lp, ln = self.engine.sequence_logprobs(tokens[:, :n].to(torch.int32), latents.to(torch.float32))
        return lp, ln.long()

    def _generate_beams(self, cond_latents, text_inputs, generate_kwargs):
        """HF generate(num_beams=K, do_sample=False) semantics (length_penalty, early_stopping False / True / "never",
        num_return_sequences = N <= K: the N best hypotheses of item b, best first, at rows b*N + j, `last_beam_scores` [B*N]; the
        repetition penalty on log-probs, pad = eos, max_length = max_gen_mel_tokens + prompt): item b is prefilled ONCE into KV slot
        b*K; every step runs [select -> KV span copies -> decode step over B*K rows] from a captured graph (include/genvc_hip.h:
        gvc_gpt_beam_generate), the host looks at the done flags once per `group` steps; the hypothesis store is finalised on the
        device at the end.  beam_length_mode: "4.33" (default: the lengths the reference's pinned transformers normalises by) or
        "generated" (those of the installed transformers).  Needs B*K <= the context's KV slots (ValueError otherwise).  Returns
        int64 [B, n] (gpt.py:609: the prompt sliced away); the best normalised score per item lands in `last_beam_scores`, and
        `last_latents` is None (the caller's latents come from the teacher-forced re-pass, hifigan_trainer.py:489-494).
        num_beam_groups = G > 1 with diversity_penalty > 0: group (diverse) beam search (include/genvc_hip.h: gvc_beam_groups,
        DESIGN.md 4.12): the K beams are G groups of K / G searched one after the other within every step, each penalised for the
        tokens the earlier groups chose at that step; the N best hypotheses over all groups are returned."""
        kw = dict(generate_kwargs)
        K, lp, rep, mode = _beam_kwargs(kw)
        N, early = _beam_returns(kw)
        G, lam = _beam_groups(kw)
        self._need_engine()
        group = int(kw.pop("group", 16))
        B = int(text_inputs.shape[0])
        if B * K > self.max_slots:
            raise ValueError(f"beam search over {B} items x {K} beams needs {B * K} KV slots; the context has {self.max_slots} "
                             "(init_gpt_for_inference(max_slots=...))")
        fake = self.compute_embeddings(cond_latents, text_inputs)
        n0 = int(fake.shape[1])
        max_new = int(kw.get("max_new_tokens") or self.max_gen_mel_tokens)                   # gpt.py:606
        dev = fake.device
        proc = logits_processors(kw, n0, self.num_audio_tokens, sampling=False)

        def run():
            slots = torch.arange(B * K, device=dev, dtype=torch.int32)
            self.engine.prefill(slots[::K].contiguous(), self._prefix, want_outputs=False)      # each item once; the first step fans out
            if G > 1:
                beam = GroupBeamSearch(fake, K, G, lam, max_new, self.stop_audio_token, self.num_audio_tokens, lp, rep, mode,
                                       early_stopping=early, **_proc_arg(proc))
            else:
                beam = BeamSearch(fake, K, max_new, self.stop_audio_token, self.num_audio_tokens, lp, rep, mode, early_stopping=early,
                                  **_proc_arg(proc))
            step = self.engine.group_beam_generate if G > 1 else self.engine.beam_generate
            while beam.steps < max_new:
                n = min(group, max_new - beam.steps)
                step(slots, beam, n, max_keys=n0 + beam.steps + n)
                stop = bool(beam.done.all().item())
                self.engine.health()          # (the .item() above synchronised)
                if stop:
                    break
            return beam.finalize(N)
        ids, scores = self._recovering(B * K, run)
        self.last_latents = None
        self.last_beam_scores = scores
        return ids

    def _generate_contrastive(self, cond_latents, text_inputs, generate_kwargs):
        """transformers 4.33 contrastive_search semantics (include/genvc_hip.h: gvc_contrastive_state): item b is prefilled ONCE into
        KV slot b*K, which also writes the ln_f rows of its prompt (the context the degeneration penalty compares with); every step runs
        [recall -> decode step over B*K rows -> hidden rows -> similarity -> select -> KV span copies] from a captured graph, the host
        looks at the finished flags once per `group` steps.  No logits warper (temperature, top_p, ... have no effect); the repetition
        penalty and the processor kwargs apply.  Needs B*K <= the context's KV slots (ValueError otherwise).  Returns int64 [B, n]
        (gpt.py:609), trimmed after the step where the last row emits the stop token as generate() trims; `last_latents` holds the
        chosen candidates' final_norm latents, as the sampling path fills it."""
        kw = dict(generate_kwargs)
        self._need_engine()
        B = int(text_inputs.shape[0])
        K, alpha, rep = _contrastive_kwargs(kw, B, self.max_slots)
        group = int(kw.pop("group", 16))
        fake = self.compute_embeddings(cond_latents, text_inputs)
        n0 = int(fake.shape[1])
        max_new = int(kw.get("max_new_tokens") or self.max_gen_mel_tokens)                   # gpt.py:606
        dev = fake.device
        proc = logits_processors(kw, n0, self.num_audio_tokens, sampling=False)

        def run():
            slots = torch.arange(B * K, device=dev, dtype=torch.int32)
            cs = ContrastiveSearch(fake, K, max_new, self.stop_audio_token, self.num_audio_tokens, self.model_dim, alpha, rep, proc=proc)
            self.engine.prefill_hidden(slots[::K].contiguous(), self._prefix, cs.hidden0)      # each item once; the first step fans out
            while cs.steps < max_new:
                n = min(group, max_new - cs.steps)
                self.engine.contrastive_generate(slots, cs, n, max_keys=n0 + cs.steps + n)
                stop = bool(cs.finished.all().item())
                self.engine.health()          # (the .item() above synchronised)
                if stop:
                    break
            return cs
        cs = self._recovering(B * K, run)
        toks = cs.tokens[:, :cs.steps].long()
        n = self._stop_len(toks)
        self.last_latents = cs.latents[:, :n]
        return toks[:, :n]

    @torch.inference_mode()
    def generate_groups(self, groups, group_kwargs=None, **generate_kwargs):
        """Several generate() calls decoded TOGETHER: groups = [(cond_latents [B_i, 32, d], text_inputs [B_i, Tc_i]), ...] with
        different code lengths.  Each group is prefilled on its own (its rows share a prefix length) into its own KV slots; the
        decode steps then run over all streams at once, so the weights stream once per step for the whole set.  Streams are
        independent, so with greedy decoding every group's result is what generate() returns for it (bit for bit when both land on
        the same decode kernels, i.e. the rows path from 5 streams up; within float rounding otherwise).  A sampling run draws class g
        with its class seed -- class_seeds[g], else seed + 7919 * g (with one shared seed all classes would draw identical per-row
        sequences) -- and by default runs the groups one after another (one generate() per group).  `joint_sampling=True` decodes them
        jointly instead, row r of group g keyed (class seed, r, tokens drawn so far): the key generate(seed=class seed) gives it, so
        each group draws what its own generate() draws from the same logits.  It is opt-in because the rows step's logits are not
        bit-identical across row counts (JOINT_SAMPLING_DEFAULT): a draw within rounding of a CDF boundary can still differ.
        `max_new_tokens` may be a list with one budget per group (benchmark mode: synthetic weights seldom stop, SURVEY.md 8d fixes
        the tokens of a segment by its duration): a group whose budget is spent leaves the joint decode, and the steps that remain
        run over the live streams only (fewer rows per step: the 8-row instead of the 16-row one-launch step for configs[2]'s tail).
        `group_kwargs` (one dict or None per group): each group's own logits processors and warpers (PROC_KWARGS, WARP_KWARGS), merged
        over the call-wide ones -- the reference runs one HF generate per segment, so they may differ between groups; each group then
        gets what generate(**its merged kwargs) returns for it, the joint decode giving every row its group's set
        (gvc_gpt_generate_proc_sets, or gvc_gpt_generate_warp when a warper is on).
        Returns a list of int64 [B_i, n_i] (reference gpt.py:594-609 per group)."""
        _plain_rows_only(generate_kwargs, "grouped (generate_groups)")
        watermark_settings(generate_kwargs, self.num_audio_tokens)          # (malformed watermarking_config: ValueError)
        _ras_on(generate_kwargs)          # (malformed ras_window / ras_threshold, or do_sample=False with them: ValueError)
        penalty_settings(generate_kwargs)          # (malformed presence_penalty / frequency_penalty / penalty_window: ValueError)
        kw = dict(generate_kwargs)
        gkw = None
        if group_kwargs is not None:
            gkw = _per_item_procs(kw, group_kwargs, len(groups), "group_kwargs", self.num_audio_tokens)
        _watermark_rows(kw, gkw, "the grouped path (generate_groups)", self.num_audio_tokens)
        self._need_engine()
        group = kw.pop("group", 16)          # decode steps per engine call (one host look at the finished flags per call)
        class_seeds = kw.pop("class_seeds", None)      # sampling runs: one seed per group (default: seed + 7919 * group index)
        joint_sampling = bool(kw.pop("joint_sampling", JOINT_SAMPLING_DEFAULT))
        budgets = kw.get("max_new_tokens")
        if isinstance(budgets, (list, tuple)):
            if len(budgets) != len(groups):
                raise ValueError(f"generate_groups: {len(budgets)} token budgets for {len(groups)} groups")
            budgets = [int(b) for b in budgets]
            kw["max_new_tokens"] = max(budgets)
        else:
            budgets = None
        # (a call with RAS on anywhere draws -- the redraw's uniform is keyed by the group's seed -- so it takes the sampling schedule
        # whatever its top_k: each group then gets what generate(seed=its class seed) returns for it)
        ras_any = _ras_on(kw) or (gkw is not None and any(ras_counts(d) is not None for d in gkw))
        greedy = (kw.get("top_k", 0) == 1 or not kw.get("do_sample", True)) and not ras_any
        total = sum(int(t.shape[0]) for _, t in groups)
        stats = getattr(self, "groups_stats", None)        # {"joint": n, "separate": n}: bench.py / tests count the two paths
        seeds = None
        if not greedy:
            # Seed semantics: class gi of THIS call draws with class_seeds[gi] when the caller numbers its classes across calls
            # (parallel_offline.convert_batch does: several calls per job), else with seed + 7919 * gi
            seeds = [int(class_seeds[gi]) if class_seeds is not None else int(kw.get("seed", 0)) + 7919 * gi for gi in range(len(groups))]
        if (not greedy and not joint_sampling) or len(groups) == 1 or total > self.max_slots or kw.get("num_beams", 1) != 1:
            if stats is not None and len(groups) > 1:
                stats["separate"] += 1
            # one generate() per class; a sampling run gives every class its own random stream (the rows of one class keep the
            # per-row numbering of the counter RNG)
            outs = []
            for gi, (c, t) in enumerate(groups):
                kg = dict(kw, **gkw[gi]) if gkw is not None else dict(kw)
                if not greedy:
                    kg["seed"] = seeds[gi]
                if budgets is not None:
                    kg["max_new_tokens"] = budgets[gi]
                outs.append(self.generate(c, t, **kg))
            self.last_latents = None      # (same contract as the joint path: callers of generate_groups want tokens)
            return outs
        return self._recovering(total, lambda: self._generate_groups_joint(groups, kw, budgets, group, stats, seeds, gkw))

    def _row_settings(self, kw):
        """the processor settings generate() would use for these kwargs (see _start), as a gvc_row_sampling entry without its key"""
        return dict(repetition_penalty=kw.get("repetition_penalty", 1.0), temperature=kw.get("temperature", 1.0),
                    top_p=kw.get("top_p", 1.0), top_k=kw.get("top_k", 0) if kw.get("do_sample", True) else 1)

    def _generate_groups_joint(self, groups, kw, budgets, group, stats, seeds=None, gkw=None):
        total = sum(int(t.shape[0]) for _, t in groups)
        if stats is not None:
            stats["joint"] += 1
        dev = groups[0][1].device
        max_new = kw.get("max_new_tokens") or self.max_gen_mel_tokens
        # rows in order of falling budget: the live streams are always the first rows of every buffer
        order = sorted(range(len(groups)), key=lambda i: -(budgets[i] if budgets else max_new))
        groups = [groups[i] for i in order]
        seeds = [seeds[i] for i in order] if seeds is not None else None
        gkw = [gkw[i] for i in order] if gkw is not None else None
        if gkw is None and ((seeds is not None and (logits_warpers(kw) is not None or ras_counts(kw) is not None))
                            or penalty_settings(kw) is not None or watermark_settings(kw, self.num_audio_tokens) is not None):
            # call-wide warpers / RAS / penalties / watermark: every group carries the call's processor, warper, RAS, penalty and
            # watermark kwargs (logits_sets; the penalties count from each group's own prompt length, greedy calls included)
            gkw = _per_item_procs(kw, [None] * len(groups), len(groups), "generate_kwargs", self.num_audio_tokens)
        gb = [budgets[i] if budgets else max_new for i in order]
        prefixes = [self.engine.prefix_embeddings(c.to(torch.float32).contiguous(), t.to(torch.int32).contiguous()) for c, t in groups]
        n0s = [int(p.shape[1]) + 1 for p in prefixes]
        width = max(n0s) + max_new + 8
        ids = torch.full((total, width), 1, device=dev, dtype=torch.int32)
        ids_len = torch.empty(total, device=dev, dtype=torch.int32)
        slots = torch.arange(total, device=dev, dtype=torch.int32)
        row = 0
        spans = []
        for p, n0 in zip(prefixes, n0s):
            b = int(p.shape[0])
            ids[row:row + b, n0 - 1] = self.start_audio_token
            ids_len[row:row + b] = n0
            self.engine.prefill(slots[row:row + b].contiguous(), p, want_outputs=False)
            spans.append((row, row + b))
            row += b
        finished = torch.zeros(total, device=dev, dtype=torch.int32)
        toks = torch.full((total, max_new), self.stop_audio_token, device=dev, dtype=torch.int32)
        lats = torch.empty(total, max_new, self.model_dim, device=dev, dtype=torch.float32)
        samp = dict(repetition_penalty=kw.get("repetition_penalty", 1.0), temperature=kw.get("temperature", 1.0),
                    top_p=kw.get("top_p", 1.0), top_k=1)
        params = sample_params(samp, self.num_audio_tokens, self.stop_audio_token, kw.get("seed", 0))
        rs = self._row_settings(kw)
        # processors: one set for the call, each row counting from its own prompt (its group's fake ids)
        proc = None
        if gkw is None and _any_proc(kw):
            plens = torch.cat([torch.full((hi - lo,), n0, dtype=torch.int32) for (lo, hi), n0 in zip(spans, n0s)]).to(dev)
            proc = logits_processors(kw, 0, self.num_audio_tokens, sampling=seeds is not None, prompt_lens=plens)
        done = 0
        while done < max_new:
            live_groups = [g for g in range(len(groups)) if gb[g] > done]
            live = spans[live_groups[-1]][1]                                   # rows [0, live) still have tokens to produce
            n = min(group, min(gb[g] for g in live_groups) - done)              # (a call never crosses the end of a budget)
            mk = max(n0s[g] for g in live_groups) + done + n
            # group_kwargs: every row its group's set, counted from its group's prompt (None: no row has a processor)
            sets = None
            if gkw is not None:
                sets = logits_sets([gkw[g] for g in live_groups for _ in range(spans[g][1] - spans[g][0])],
                                   [n0s[g] for g in live_groups for _ in range(spans[g][1] - spans[g][0])],
                                   self.num_audio_tokens, sampling=seeds is not None, engine=self.engine)
            # sampling: row r of class g is keyed (class seed, r, done) -- what generate(seed=class seed) draws for it
            rows = None
            if seeds is not None:
                rows = [dict(rs, seed=seeds[g], rng_row=r, rng_step0=done) for g in live_groups for r in range(spans[g][1] - spans[g][0])]
            _generate_call(self.engine, slots[:live], ids[:live], ids_len[:live], finished[:live], params, done, n, toks[:live], lats[:live],
                           max_keys=mk, rows=rows, proc=proc, sets=sets)
            done += n
            stop = bool(finished[:live].all().item())
            self.engine.health()
            if stop:
                break
        out = [None] * len(groups)
        for g, (lo, hi) in enumerate(spans):
            t = toks[lo:hi, :min(done, gb[g])].long()
            out[order[g]] = t[:, :self._stop_len(t)]
        self.last_latents = None          # (per-group latents are not kept: the callers of this path want tokens)
        return out

    @torch.inference_mode()
    def generate_rolling(self, jobs, job_kwargs=None, **generate_kwargs):
        """generate_groups with a ROLLING set of streams: jobs = [(cond_latents [B_i, 32, d], text_inputs
        [B_i, Tc_i]), ...] are admitted in order as KV slots become free.  Retirement is PER ROW, as the reference's loop tracks
        `unfinished_sequences` per row (stream_generator.py:861-874): a row that has emitted the stop token gives its KV slot back at
        the next host look (every `group` steps) and stops taking a row of the decode step; the rows of a job whose budget is spent
        leave together.  Freed slots go to the next job as soon as all ITS rows fit, so the decode step stays full instead of
        draining to the longest stream (configs[2]: the 47-step tail of a micro-batch's 6 s class runs beside the NEXT micro-batch's
        4 s class; a real checkpoint ends every class ragged).  Streams are independent given their prefix, so every job gets what
        generate() returns for it: finished rows padded with the stop token up to the step where the job's last row stops
        (reference gpt.py:594-609).  `max_new_tokens`: one budget, or a list with one per job.  Returns a list of int64 [B_i, n_i]
        in job order.  `self.rolling_stats` (if the attribute is a dict) accumulates row_steps_issued / row_steps_live: rows x steps
        the decode calls ran, and how many of them produced a token the reference's loop would have produced.
        Sampling (top_k != 1) needs `job_seeds`, one per job: row r of job j is keyed (job_seeds[j], r, tokens job j has drawn), so
        job j draws what generate(c_j, t_j, seed=job_seeds[j]) draws from the same logits, whatever it shares the decode step with (the
        rows step's logits themselves are not bit-identical across row counts: JOINT_SAMPLING_DEFAULT).  Without job_seeds a sampling
        call raises NotImplementedError.
        `job_kwargs` (one dict or None per job): each job's own logits processors and warpers (PROC_KWARGS, WARP_KWARGS), merged over
        the call-wide ones; job j then gets what generate(c_j, t_j, **its merged kwargs) returns (seed=job_seeds[j] when sampling), each
        row of a decode call carrying its job's set (gvc_gpt_generate_proc_sets, or gvc_gpt_generate_warp when a warper is on)."""
        _plain_rows_only(generate_kwargs, "rolling (generate_rolling)")
        watermark_settings(generate_kwargs, self.num_audio_tokens)          # (malformed watermarking_config: ValueError)
        _ras_on(generate_kwargs)          # (malformed ras_window / ras_threshold, or do_sample=False with them: ValueError)
        penalty_settings(generate_kwargs)          # (malformed presence_penalty / frequency_penalty / penalty_window: ValueError)
        kw = dict(generate_kwargs)
        jkw = None
        if job_kwargs is not None:
            jkw = _per_item_procs(kw, job_kwargs, len(jobs), "job_kwargs", self.num_audio_tokens)
        _watermark_rows(kw, jkw, "the rolling path (generate_rolling)", self.num_audio_tokens)
        self._need_engine()
        group = kw.pop("group", 16)
        kw.pop("class_seeds", None)
        job_seeds = kw.pop("job_seeds", None)
        max_rows = kw.pop("max_rows", None)      # streams in flight at most (default: every KV slot of the context)
        ras_any = _ras_on(kw) or (jkw is not None and any(ras_counts(d) is not None for d in jkw))
        greedy = (kw.get("top_k", 0) == 1 or not kw.get("do_sample", True)) and not ras_any      # (RAS draws: it needs the jobs' seeds)
        if (not greedy and job_seeds is None) or kw.get("num_beams", 1) != 1:
            raise NotImplementedError("generate_rolling samples with one seed per job (job_seeds=...); without them it serves greedy "
                                      "decoding (top_k = 1) only")
        if job_seeds is not None and len(job_seeds) != len(jobs):
            raise ValueError(f"generate_rolling: {len(job_seeds)} job seeds for {len(jobs)} jobs")
        budgets = kw.get("max_new_tokens")
        if isinstance(budgets, (list, tuple)):
            if len(budgets) != len(jobs):
                raise ValueError(f"generate_rolling: {len(budgets)} token budgets for {len(jobs)} jobs")
            budgets = [int(b) for b in budgets]
        else:
            budgets = [int(budgets or self.max_gen_mel_tokens)] * len(jobs)
        if not jobs:
            return []
        n0s = [int(t.shape[1]) + int(c.shape[1]) + 3 for c, t in jobs]            # prefix rows (cond + text + 2) + the start token
        width = max(n0 + b for n0, b in zip(n0s, budgets)) + 8
        S = min(self.max_slots, int(max_rows)) if max_rows else self.max_slots
        if max(int(t.shape[0]) for _, t in jobs) > S:
            raise ValueError(f"generate_rolling: a job has more rows than streams may be in flight ({S}; KV slots {self.max_slots})")
        seeds = None if greedy else [int(x) for x in job_seeds]
        return self._recovering(S, lambda: self._rolling(jobs, kw, budgets, group, n0s, width, S, seeds, jkw))

    def _rolling(self, jobs, kw, budgets, group, n0s, width, S, seeds=None, jkw=None):
        dev = jobs[0][1].device
        if jkw is None and ((seeds is not None and (logits_warpers(kw) is not None or ras_counts(kw) is not None))
                            or penalty_settings(kw) is not None or watermark_settings(kw, self.num_audio_tokens) is not None):
            # call-wide warpers / RAS / penalties / watermark: every job carries the call's processor, warper, RAS and penalty kwargs
            # (logits_sets; the penalties count from each job's own prompt length, greedy calls included)
            jkw = _per_item_procs(kw, [None] * len(jobs), len(jobs), "generate_kwargs", self.num_audio_tokens)
        eng = self.engine
        stop = self.stop_audio_token
        ids_all = torch.ones(S, width, device=dev, dtype=torch.int32)
        len_all = torch.zeros(S, device=dev, dtype=torch.int32)
        fin_all = torch.zeros(S, device=dev, dtype=torch.int32)
        samp = dict(repetition_penalty=kw.get("repetition_penalty", 1.0), temperature=kw.get("temperature", 1.0),
                    top_p=kw.get("top_p", 1.0), top_k=1)
        params = sample_params(samp, self.num_audio_tokens, stop, kw.get("seed", 0))
        rs = self._row_settings(kw)
        stats = getattr(self, "groups_stats", None)
        rstats = getattr(self, "rolling_stats", None)
        free = list(range(S))
        live, out, nxt = [], [None] * len(jobs), 0
        while nxt < len(jobs) or live:
            # admit jobs in order while all their rows fit
            while nxt < len(jobs) and int(jobs[nxt][1].shape[0]) <= len(free):
                c, t = jobs[nxt]
                b = int(t.shape[0])
                mine = free[:b]
                del free[:b]
                sl = torch.tensor(mine, device=dev, dtype=torch.int32)
                prefix = eng.prefix_embeddings(c.to(torch.float32).contiguous(), t.to(torch.int32).contiguous())
                eng.prefill(sl, prefix, want_outputs=False)
                idx = sl.long()
                ids_all[idx] = 1                                    # (a reused slot starts with a clean history: repetition_penalty reads it)
                ids_all[idx, n0s[nxt] - 1] = self.start_audio_token
                len_all[idx] = n0s[nxt]
                fin_all[idx] = 0
                live.append(dict(job=nxt, slots=mine, alive=list(range(b)), n0=n0s[nxt], budget=budgets[nxt], done=0,
                                 toks=torch.full((b, budgets[nxt]), stop, device=dev, dtype=torch.int32)))
                nxt += 1
            n = min(group, min(j["budget"] - j["done"] for j in live))
            row_slots = [j["slots"][r] for j in live for r in j["alive"]]
            rows = torch.tensor(row_slots, device=dev, dtype=torch.int32)
            idx = rows.long()
            W = max(j["n0"] + j["done"] for j in live) + n + 8
            ids = ids_all[idx, :W].contiguous()
            ids_len = len_all[idx].contiguous()
            fin = fin_all[idx].contiguous()
            toks = torch.full((len(row_slots), n), stop, device=dev, dtype=torch.int32)
            # processors: one set for the call, each row counting from its own job's prompt
            proc = sets = None
            if jkw is not None:
                # job_kwargs: every row its job's set, counted from its job's prompt (None: no row has a processor)
                sets = logits_sets([jkw[j["job"]] for j in live for _ in j["alive"]], [j["n0"] for j in live for _ in j["alive"]],
                                   self.num_audio_tokens, sampling=seeds is not None, engine=self.engine)
            elif _any_proc(kw):
                plens = torch.tensor([j["n0"] for j in live for _ in j["alive"]], dtype=torch.int32).to(dev)
                proc = logits_processors(kw, 0, self.num_audio_tokens, sampling=seeds is not None, prompt_lens=plens)
            # row r of job j keyed (job seed, r, tokens the job has drawn): the key generate(seed=job_seeds[j]) gives that row
            keys = None
            if seeds is not None:
                keys = [dict(rs, seed=seeds[j["job"]], rng_row=r, rng_step0=j["done"]) for j in live for r in j["alive"]]
            _generate_call(eng, rows, ids, ids_len, fin, params, 0, n, toks, None, max_keys=W - 8, rows=keys, proc=proc, sets=sets)
            ids_all[idx, :W] = ids
            len_all[idx] = ids_len
            fin_all[idx] = fin
            fin_h = fin.cpu()                                      # (synchronises)
            eng.health()
            if stats is not None:
                stats["joint"] += 1
            if rstats is not None:
                th = toks.cpu()
                hit = th == stop
                first = torch.where(hit.any(1), hit.int().argmax(1) + 1, torch.full((th.shape[0],), n))
                rstats["row_steps_issued"] = rstats.get("row_steps_issued", 0) + n * len(row_slots)
                rstats["row_steps_live"] = rstats.get("row_steps_live", 0) + int(first.sum())
                rstats["calls"] = rstats.get("calls", 0) + 1
            r = 0
            keep = []
            for j in live:
                k = len(j["alive"])
                a = torch.tensor(j["alive"], device=dev, dtype=torch.long)
                j["toks"][a, j["done"]:j["done"] + n] = toks[r:r + k]
                j["done"] += n
                still = [row for i, row in enumerate(j["alive"]) if not bool(fin_h[r + i])]
                gone = [row for i, row in enumerate(j["alive"]) if bool(fin_h[r + i])]
                r += k
                if j["done"] >= j["budget"] or not still:           # the job is over: its budget is spent or its last row has stopped
                    t = j["toks"][:, :j["done"]].long()
                    out[j["job"]] = t[:, :self._stop_len(t)]
                    gone = j["alive"]
                else:
                    j["alive"] = still
                    keep.append(j)
                free.extend(j["slots"][row] for row in gone)        # a stopped row's slot serves the next job from the next call on
                free.sort()
            live = keep
        self.last_latents = None
        return out

    def _stop_len(self, toks):
        """steps the reference loop runs: up to and including the step where the last row emits the stop token"""
        is_stop = toks == self.stop_audio_token
        if not bool(is_stop.any(1).all()):
            return toks.shape[1]
        return int(is_stop.long().argmax(1).max().item()) + 1

    @torch.inference_mode()
    def get_generator(self, fake_inputs, **generate_kwargs):
        """reference gpt.py:612-621 + stream_generator.py:865: yields (tokens int64[B], latent float[B,d]) per step,
        the EOS step included.  Steps run in groups of `stream_group` (default 8, the vocoder chunk of
        inference_utils.py:195) with one host check of the finished flags per group."""
        _plain_rows_only(generate_kwargs, "streaming (get_generator)")
        _watermark(generate_kwargs, self.num_audio_tokens)          # (malformed or refused watermarking_config: raised before any work)
        _ras_on(generate_kwargs)          # (malformed ras_window / ras_threshold, or do_sample=False with them: ValueError)
        penalty_settings(generate_kwargs)          # (malformed presence_penalty / frequency_penalty / penalty_window: ValueError)
        self._need_engine()
        group = generate_kwargs.pop("stream_group", 8)
        B = int(fake_inputs.shape[0])
        emitted = 0
        st = None
        retried = False

        def restart():
            # a hand-off time-out (see _recovering): the segment is generated again from its start on the launch-per-phase paths --
            # a full prefill (the reset slots have lost their cached conditioning rows) -- and the steps already yielded are skipped:
            # greedy decoding repeats them (with top_k > 1 what follows comes from a different token sequence)
            self.recoveries = getattr(self, "recoveries", 0) + 1
            torch.cuda.synchronize()
            self.engine.reset(torch.arange(B, device=fake_inputs.device, dtype=torch.int32))
            s2 = self._start(fake_inputs, dict(generate_kwargs, cached_cond_rows=0))
            while s2["done"] < emitted and not self._advance(s2, min(group, emitted - s2["done"])):
                pass
            return s2
        try:
            while True:
                try:
                    if st is None:
                        st = self._start(fake_inputs, generate_kwargs)
                    end = self._advance(st, group)
                except GenvcHipError as e:
                    if not e.is_handoff_timeout or retried:
                        raise
                    retried = True
                    st = restart()
                    continue
                toks = st["toks"][:, emitted:st["done"]].long()
                n = toks.shape[1]
                if end and n:
                    n = min(n, self._stop_len(st["toks"][:, :st["done"]].long()) - emitted)
                for i in range(n):
                    yield toks[:, i], st["lats"][:, emitted + i]
                emitted += n
                if end:
                    return
        finally:
            # (the generator ended, was closed or collected: its table's slot in the engine's arena is free for others)
            if st is not None and st.get("wm") is not None:
                st["wm"].release()

    def inference(self, cond_latents, text_inputs, **generate_kwargs):
        return self.generate(cond_latents, text_inputs, **generate_kwargs)

    @torch.inference_mode()
    def forward(self, text_inputs, text_lengths, audio_codes, wav_lengths, cond_mels=None, cond_lens=None,
                cond_latents=None, return_attentions=False, return_latent=False):
        """reference gpt.py:375-537 in eval mode.
        Default call: a padded batch with `text_lengths`, `wav_lengths` (samples) and `cond_mels` (b,1,80,s) + `cond_lens` (samples; or
        `cond_latents` (b,32,d) alone) -> (loss_text, loss_mel, Top10Accuracy, mel_logits [B, V, Lm]): the evaluation pass
        (forward_eval_prepare on the host, then gvc_gpt_forward_rows + gvc_gpt_head_xent).  Top10Accuracy follows the published
        definition of torchmetrics MulticlassAccuracy(top_k=10, average="micro", ignore_index=-1).
        `return_latent=True` with `cond_latents` (inference_utils.py:71-76) -> latents [B,n,d] of the n = max ceil(wav_lengths/1024) codes;
        ragged lengths take the reference's padding and no attention mask (gpt.py:450)."""
        self._need_engine()
        if return_attentions:
            raise NotImplementedError("return_attentions: the attention kernels do not keep their weights (GPT.trace runs a pass "
                                      "that does, for given codes)")
        dev = audio_codes.device
        if return_latent and cond_latents is not None:
            B, n = audio_codes.shape
            if int(text_lengths.min()) == text_inputs.shape[1] and int(torch.ceil(wav_lengths / self.code_stride_len).min()) == n:
                prefix = self.engine.prefix_embeddings(cond_latents.to(torch.float32).contiguous(),
                                                       text_inputs.to(torch.int32).contiguous())
                slots = torch.arange(B, device=dev, dtype=torch.int32)
                return self.engine.latents(slots, prefix, audio_codes.to(torch.int32).contiguous())
        # everything below is new ground (the equal-length re-pass above serves a module in either mode, as it always has)
        if self.training:
            raise NotImplementedError("GPT.forward in training mode (dropout, gradients, [:, :-1] latents): call .eval() first")
        if self.train_solo_embeddings or self.average_conditioning_embeddings:
            raise NotImplementedError("train_solo_embeddings / average_conditioning_embeddings are not part of the evaluation pass")
        if cond_latents is None and cond_mels is None:
            raise ValueError("forward: cond_mels (with cond_lens) or cond_latents is needed")
        if cond_latents is None:
            cond_latents = self.get_style_emb(cond_mels, seq_lens=None if cond_lens is None else
                                              torch.as_tensor(cond_lens).to("cpu") // self.perceiver_cond_length_compression)   # gpt.py:407-408, 486
            cond_latents = cond_latents.transpose(1, 2)
        cond_latents = cond_latents.to(device=dev, dtype=torch.float32).contiguous()
        prep = forward_eval_prepare(text_inputs, text_lengths, audio_codes, wav_lengths, code_stride_len=self.code_stride_len,
                                    start_text_token=self.start_text_token, stop_text_token=self.stop_text_token,
                                    start_audio_token=self.start_audio_token, stop_audio_token=self.stop_audio_token,
                                    number_text_tokens=self.number_text_tokens, num_audio_tokens=self.num_audio_tokens,
                                    n_cond=cond_latents.shape[1])
        B, Lt = prep["text_ids"].shape
        Lm = prep["code_ids"].shape[1]
        if B > self.max_slots:
            raise ValueError(f"forward: {B} items exceed the context's {self.max_slots} slots (init_gpt_for_inference(max_slots=))")
        slots = torch.arange(B, device=dev, dtype=torch.int32)
        text_ids, code_ids = prep["text_ids"].to(dev, torch.int32), prep["code_ids"].to(dev, torch.int32)
        key_mask = None if return_latent else prep["key_mask"].to(dev, torch.uint8)           # gpt.py:450
        lat = self.engine.forward_rows(slots, cond_latents, text_ids, code_ids, key_mask)
        if return_latent:
            return lat[:, Lt:][:, :-5].contiguous()                                           # gpt.py:304, 491, 508
        _, _, s_text = self.engine.head_xent(lat[:, :Lt].reshape(B * Lt, -1), "text", prep["text_targets"].reshape(-1).to(dev, torch.int32),
                                             self.label_smoothing)
        mel_logits, _, s_mel = self.engine.head_xent(lat[:, Lt:].reshape(B * Lm, -1), "mel",
                                                     prep["mel_targets"].reshape(-1).to(dev, torch.int32), self.label_smoothing)
        loss_text, loss_mel = s_text[0].to(torch.float32), s_mel[0].to(torch.float32)
        acc = (s_mel[1] / s_mel[2]).to(torch.float32)
        return loss_text, loss_mel, acc, mel_logits.view(B, Lm, -1).permute(0, 2, 1)
