"""ctypes binding of libgenvc_hip.so (include/genvc_hip.h).

The product path has NO CPU fallback: if the library is missing or a call fails this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GENVC_HIP_LIB") or os.path.join(_HERE, "lib", "libgenvc_hip.so")     # override: A/B runs of two builds

c_i32p = C.POINTER(C.c_int32)
c_f32p = C.POINTER(C.c_float)


class GptDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_layer", "d_model", "n_head", "vocab", "max_mel_pos", "max_text_pos",
                                         "n_text", "max_seq", "max_slots", "max_rows", "weight_dtype")]


class SampleParams(C.Structure):
    _fields_ = [("repetition_penalty", C.c_float), ("temperature", C.c_float), ("top_p", C.c_float),
                ("top_k", C.c_int32), ("eos_token", C.c_int32), ("vocab", C.c_int32), ("seed", C.c_uint64)]


class RowSampling(C.Structure):
    """gvc_row_sampling: per-row sampling settings and RNG key (32 bytes; layout fixed in include/genvc_hip.h)"""
    _fields_ = [("repetition_penalty", C.c_float), ("temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32),
                ("seed", C.c_uint64), ("rng_row", C.c_int32), ("rng_step0", C.c_int32)]


class BeamState(C.Structure):
    """gvc_beam_state (include/genvc_hip.h): sizes, settings and the device arrays of one beam search"""
    _fields_ = [(n, C.c_int32) for n in ("B", "K", "vocab", "eos", "n0", "ids_stride", "max_new", "length_mode")] + \
        [("length_penalty", C.c_float), ("repetition_penalty", C.c_float)] + \
        [(n, C.c_void_p) for n in ("ids", "scores", "tokens", "parents", "done", "hyp_score", "hyp_len", "hyp_tok", "hyp_count",
                                   "hyp_worst", "copies", "n_copies")]


class BeamGroups(C.Structure):
    """gvc_beam_groups (include/genvc_hip.h): the groups of a group (diverse) beam search and their per-(item, group) device arrays"""
    _fields_ = [("G", C.c_int32), ("diversity_penalty", C.c_float)] + [(n, C.c_void_p) for n in ("done", "hyp_count", "hyp_worst")]


class ContrastiveState(C.Structure):
    """gvc_contrastive_state (include/genvc_hip.h): sizes, settings and the device arrays of one contrastive search"""
    _fields_ = [(n, C.c_int32) for n in ("B", "K", "vocab", "eos", "n0", "ids_stride", "max_new")] + \
        [("penalty_alpha", C.c_float), ("repetition_penalty", C.c_float), ("reserved", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("ids", "finished", "tokens_out", "latents_out", "hidden0")]


class LogitsProcessors(C.Structure):
    """gvc_logits_processors (include/genvc_hip.h): one call's length / repetition processors; all zero = every processor off"""
    _fields_ = [(n, C.c_int32) for n in ("no_repeat_ngram_size", "min_length", "min_new_tokens", "decay_start")] + \
        [("decay_factor", C.c_float), ("min_p", C.c_float)] + \
        [(n, C.c_int32) for n in ("prompt_len", "n_suppress", "n_begin_suppress", "reserved")] + \
        [("prompt_lens", C.c_void_p), ("suppress", C.c_uint32 * 33), ("begin_suppress", C.c_uint32 * 33)]


class LogitsWarpers(C.Structure):
    """gvc_logits_warpers (include/genvc_hip.h): typical / epsilon / eta sampling warpers of one set (16 bytes); 0 = off"""
    _fields_ = [("typical_p", C.c_float), ("epsilon_cutoff", C.c_float), ("eta_cutoff", C.c_float), ("reserved", C.c_int32)]


RAS_MAX_WINDOW = 64                  # GVC_RAS_MAX_WINDOW
RAS_SALT = 0x5241535F52454452        # GVC_RAS_SALT: the redraw's uniform is rng_uniform(seed ^ RAS_SALT, step, row)


class LogitsRas(C.Structure):
    """gvc_logits_ras (include/genvc_hip.h): repetition-aware sampling of one set (16 bytes); window 0 = off"""
    _fields_ = [(n, C.c_int32) for n in ("window", "min_count", "prompt_len", "reserved")]


PENALTY_MAX = 2.0                    # GVC_PENALTY_MAX: |presence|, |frequency| <= 2


class LogitsPenalties(C.Structure):
    """gvc_logits_penalties (include/genvc_hip.h): presence / frequency / windowed repetition penalties of one set (16 bytes);
    presence == frequency == 0 and window == 0: off"""
    _fields_ = [("presence", C.c_float), ("frequency", C.c_float), ("window", C.c_int32), ("prompt_len", C.c_int32)]


WM_LEFTHASH, WM_SELFHASH = 0, 1      # GVC_WM_LEFTHASH, GVC_WM_SELFHASH
WM_SELFHASH_TOP = 40                 # GVC_WM_SELFHASH_TOP
WM_MAX_SCORE_LEN = 8192              # gvc_wm_score: codes per row


class LogitsWatermark(C.Structure):
    """gvc_logits_watermark (include/genvc_hip.h): the green-list watermark of one set (24 bytes): a device table, the bias, the
    scheme and the words of a table row; a null table: off"""
    _fields_ = [("table", C.c_void_p), ("bias", C.c_float), ("scheme", C.c_int32), ("words", C.c_int32), ("reserved", C.c_int32)]


BIAS_MAX_SEQS = 32     # GVC_BIAS_MAX_SEQS
BIAS_MAX_LEN = 8       # GVC_BIAS_MAX_LEN


class LogitsBias(C.Structure):
    """gvc_logits_bias (include/genvc_hip.h): one call's sequence bias, bad words, forced EOS and renormalize flag (1312 bytes); all
    zero = off"""
    _fields_ = [(n, C.c_int32) for n in ("n_bias", "n_ban", "force_eos_at", "renormalize", "prompt_len")] + \
        [("reserved", C.c_int32 * 3), ("len", C.c_int32 * BIAS_MAX_SEQS), ("bias", C.c_float * BIAS_MAX_SEQS),
         ("ids", (C.c_int32 * BIAS_MAX_LEN) * BIAS_MAX_SEQS)]


class SpecState(C.Structure):
    """gvc_spec_state (include/genvc_hip.h): sizes and the device arrays of one assisted (speculative) generation"""
    _fields_ = [(n, C.c_int32) for n in ("B", "ids_stride", "max_new", "tok_stride", "lat_stride", "d")] + \
        [(n, C.c_void_p) for n in ("ids", "ids_len", "finished", "emitted", "pending", "toks", "lats", "drop_target", "drop_assistant",
                                   "rounds", "drafted", "accepted", "v_toks", "v_logits", "v_latents", "d_ids_len", "d_finished")]


class SpecSampling(C.Structure):
    """gvc_spec_sampling (include/genvc_hip.h): the device workspaces of a sampled assisted generation (24 bytes)"""
    _fields_ = [(n, C.c_void_p) for n in ("q_scores", "p_scores", "rows")]


class PerceiverDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim", "depth", "dim_context", "num_latents", "dim_head", "heads",
                                         "ff_mult", "max_batch", "max_frames")]


class DvaeDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("channels", "hidden_dim", "num_layers", "num_resnet_blocks", "kernel_size",
                                         "codebook_dim", "num_tokens", "max_batch", "max_frames")]


DVAE_DECODER = 1          # GVC_DVAE_DECODER (gvc_dvae_create_ex)


class DiscDims(C.Structure):
    """gvc_disc_dims (include/genvc_hip.h): one waveform-domain discriminator (MSD or MPD)"""
    _fields_ = [("kind", C.c_int32), ("n_sub", C.c_int32), ("periods", C.c_int32 * 8), ("channels", C.c_int32 * 5),
                ("spectral_norm", C.c_int32), ("max_batch", C.c_int32), ("max_samples", C.c_int32)]


DISC_MSD, DISC_MPD = 0, 1                                        # GVC_DISC_MSD, GVC_DISC_MPD
MEL_SLANEY_SCALE, MEL_MAGNITUDE, MEL_PAD_HALF_OVERLAP = 1, 2, 4  # GVC_MEL_* (gvc_mel_create_ex)


class MelOptions(C.Structure):
    """gvc_mel_options (include/genvc_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("n_fft", "hop", "win", "sample_rate", "n_mels", "flags")] + \
        [("f_min", C.c_float), ("f_max", C.c_float), ("mel_norms_host", C.POINTER(C.c_float))]


class GlOptions(C.Structure):
    """gvc_gl_options (include/genvc_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("n_fft", "hop", "win", "sample_rate", "n_mels", "max_batch", "max_frames")] + \
        [("f_min", C.c_float), ("f_max", C.c_float)]


class TraceOptions(C.Structure):
    """gvc_trace_options (include/genvc_hip.h)"""
    _fields_ = [(n, C.c_int32) for n in ("start_tok", "stop_tok", "content_off", "n_content")] + [("layer_mask", C.c_uint64)] + \
        [(n, C.c_void_p) for n in ("probs", "hidden", "align", "scratch")]


class HifiganDims(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("up_init_ch", C.c_int32), ("n_ups", C.c_int32), ("up_rates", C.c_int32 * 4),
                ("up_kernels", C.c_int32 * 4), ("n_kernels", C.c_int32), ("res_kernels", C.c_int32 * 4),
                ("res_dilations", (C.c_int32 * 2) * 4), ("max_batch", C.c_int32), ("max_frames", C.c_int32)]


class HifiganDimsEx(C.Structure):
    """gvc_hifigan_dims_ex (include/genvc_hip.h): HifiganDims plus resblock_type and a third dilation per kernel"""
    _fields_ = [("in_dim", C.c_int32), ("up_init_ch", C.c_int32), ("n_ups", C.c_int32), ("up_rates", C.c_int32 * 4),
                ("up_kernels", C.c_int32 * 4), ("n_kernels", C.c_int32), ("res_kernels", C.c_int32 * 4), ("resblock_type", C.c_int32),
                ("res_dilations", (C.c_int32 * 3) * 4), ("max_batch", C.c_int32), ("max_frames", C.c_int32)]


class HubertDims(C.Structure):
    _fields_ = [("n_conv", C.c_int32), ("conv_dim", C.c_int32 * 8), ("conv_kernel", C.c_int32 * 8),
                ("conv_stride", C.c_int32 * 8)] + [(n, C.c_int32) for n in (
                    "embed_dim", "n_layers", "n_heads", "ffn_dim", "pos_conv_kernel", "pos_conv_groups", "final_dim",
                    "max_batch", "max_samples")]


class GemmCase(C.Structure):
    """gvc_gemm_case (include/genvc_hip.h): one launch of one fp32 GEMM kernel class on caller-owned device buffers (test hook)"""
    _fields_ = [(n, C.c_int32) for n in ("kind", "M", "N", "K")] + \
        [(n, C.c_void_p) for n in ("A", "W", "C", "work")] + \
        [(n, C.c_int64) for n in ("a_batch_stride", "a_batch_stride2", "w_batch_stride", "c_batch_stride", "c_batch_stride2", "work_cap")] + \
        [(n, C.c_int32) for n in ("lda", "ldw", "ldc", "w_bf16", "batch", "batch_inner", "conv_cin", "conv_tap_stride", "a_act")] + \
        [("a_slope", C.c_float), ("att_part", C.c_void_p)] + \
        [(n, C.c_int32) for n in ("att_nc", "att_heads", "att_hd", "sk", "raw_partials", "mtw", "sk_used")] + \
        [(n, C.c_void_p) for n in ("bias", "resid", "resid2")] + \
        [(n, C.c_int64) for n in ("bias_batch_stride", "resid_batch_stride", "resid_batch_stride2")] + \
        [(n, C.c_int32) for n in ("act", "ldr", "resid_fm16", "geglu", "c_fm16", "qkv", "d", "n_head", "head_dim", "max_seq", "T",
                                  "kv_bf16")] + \
        [("out_scale", C.c_float), ("reserved", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("kcache", "vcache", "slots", "base_len", "x_in", "x_out", "part", "pbias", "ln_w", "ln_b", "stats")] + \
        [("ln_sk", C.c_int32), ("ln_rows", C.c_int32)]


# gvc_gemm_case.kind (GVC_GEMM_*)
GEMM_TILED, GEMM_SKINNY, GEMM_SKINNY_LN, GEMM_STRIP, GEMM_STRIP_GEOM, GEMM_LN_ROWS, GEMM_LN_ROWS_B16, GEMM_TO_FM16, GEMM_TO_FM16_BF16 = range(9)

class AttnCase(C.Structure):
    """gvc_attn_case (include/genvc_hip.h): one launch of one attention kernel class on caller-owned device buffers (test hook)"""
    _fields_ = [(n, C.c_int32) for n in ("kind", "head_dim", "n_head", "kv_bf16")] + \
        [(n, C.c_void_p) for n in ("q", "kbase", "vbase")] + \
        [(n, C.c_int64) for n in ("k_batch_stride", "k_head_stride")] + \
        [(n, C.c_int32) for n in ("q_stride", "k_row_stride", "T", "causal", "n_keys", "out_stride", "out_fm16", "mask_stride")] + \
        [("scale", C.c_float), ("reserved", C.c_int32)] + \
        [(n, C.c_void_p) for n in ("slots", "base_len", "out", "key_mask")] + \
        [(n, C.c_int32) for n in ("chunks", "rows", "direct", "wide", "batch", "max_keys", "taken", "ran")] + \
        [(n, C.c_void_p) for n in ("seq_len", "Wp")] + \
        [(n, C.c_int32) for n in ("max_seq", "d", "nw", "mask")] + \
        [("fmask", C.c_void_p), ("ld", C.c_int64), ("bs", C.c_int64)] + \
        [(n, C.c_int32) for n in ("Tq", "Tk", "out_rows", "E")]


# gvc_attn_case.kind (GVC_ATTN_*) and .ran (GVC_ATTN_RAN_*)
ATTN_ROWS, ATTN_TILE, ATTN_TILE_MASKED, ATTN_FUSED_PROJ, ATTN_64 = range(5)
ATTN_RAN_NONE, ATTN_RAN_SHORT, ATTN_RAN_TILED = range(3)

_P = C.c_void_p
_SIGNATURES = {
    "gvc_version": (C.c_int, []),
    "gvc_last_error": (C.c_char_p, []),
    "gvc_gpt_create": (C.c_int, [C.POINTER(GptDims), C.POINTER(_P)]),
    "gvc_gpt_destroy": (C.c_int, [_P]),
    "gvc_gpt_bind_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "gvc_gpt_missing_weights": (C.c_int, [_P]),
    "gvc_gpt_prefix_embeddings": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "gvc_gpt_prefill": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_gpt_prefill_cached": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_gpt_prefill_cond": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P]),
    "gvc_gpt_decode_step": (C.c_int, [_P, _P, C.c_int32, _P, _P, _P, _P]),
    "gvc_gpt_reset_slots": (C.c_int, [_P, _P, C.c_int32, _P]),
    "gvc_gpt_kv_fanout": (C.c_int, [_P, _P, _P, C.c_int32, _P]),
    "gvc_gpt_sequence_logprobs": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "gvc_gpt_latents": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "gvc_gpt_trace": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(TraceOptions), _P]),
    "gvc_gpt_forward_rows": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "gvc_gpt_head_xent": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_float, C.c_int32, _P, _P, _P, _P]),
    "gvc_sample": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.c_int32, _P, _P]),
    "gvc_gpt_generate": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.c_int32,
                                   C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P]),
    "gvc_sample_rows": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                  C.c_int32, _P, _P]),
    "gvc_gpt_generate_rows": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                        C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P]),
    "gvc_beam_select": (C.c_int, [C.POINTER(BeamState), _P, _P, C.c_int32, _P]),
    "gvc_gpt_beam_generate": (C.c_int, [_P, _P, C.POINTER(BeamState), C.c_int32, C.c_int32, C.c_int32, _P]),
    "gvc_gpt_warmup_beam": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32]),
    "gvc_sample_proc": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                  C.POINTER(LogitsProcessors), C.c_int32, _P, _P]),
    "gvc_gpt_generate_proc": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                        C.POINTER(LogitsProcessors), C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32,
                                        _P]),
    "gvc_beam_select_proc": (C.c_int, [C.POINTER(BeamState), C.POINTER(LogitsProcessors), _P, _P, C.c_int32, _P]),
    "gvc_gpt_beam_generate_proc": (C.c_int, [_P, _P, C.POINTER(BeamState), C.POINTER(LogitsProcessors), C.c_int32, C.c_int32,
                                             C.c_int32, _P]),
    "gvc_group_beam_select": (C.c_int, [C.POINTER(BeamState), C.POINTER(BeamGroups), C.POINTER(LogitsProcessors), _P, _P, C.c_int32, _P]),
    "gvc_gpt_group_beam_generate": (C.c_int, [_P, _P, C.POINTER(BeamState), C.POINTER(BeamGroups), C.POINTER(LogitsProcessors),
                                              C.c_int32, C.c_int32, C.c_int32, _P]),
    "gvc_gpt_warmup_group_beam": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gvc_gpt_prefill_hidden": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, C.c_int32, _P, _P]),
    "gvc_gpt_contrastive_generate": (C.c_int, [_P, _P, C.POINTER(ContrastiveState), C.c_int32, C.c_int32, C.c_int32, _P]),
    "gvc_gpt_contrastive_generate_proc": (C.c_int, [_P, _P, C.POINTER(ContrastiveState), C.POINTER(LogitsProcessors), C.c_int32,
                                                    C.c_int32, C.c_int32, _P]),
    "gvc_gpt_warmup_contrastive": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32]),
    "gvc_sample_proc_sets": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                       C.POINTER(LogitsProcessors), C.c_int32, c_i32p, C.c_int32, _P, _P]),
    "gvc_gpt_generate_proc_sets": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                             C.POINTER(LogitsProcessors), C.c_int32, c_i32p, C.c_int32, C.c_int32, C.c_int32, _P,
                                             C.c_int32, _P, C.c_int32, _P]),
    "gvc_sample_warp": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                  C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p, C.c_int32, _P, _P]),
    "gvc_gpt_generate_warp": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                        C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p, C.c_int32, C.c_int32,
                                        C.c_int32, _P, C.c_int32, _P, C.c_int32, _P]),
    "gvc_cfg_guide": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_float, _P, _P]),
    "gvc_gpt_generate_cfg": (C.c_int, [_P, _P, _P, C.c_int32, C.c_float, _P, C.c_int32, _P, _P, C.POINTER(SampleParams),
                                       C.POINTER(RowSampling), C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p,
                                       C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P]),
    "gvc_gpt_warmup_cfg": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32]),
    "gvc_gpt_generate_scores": (C.c_int, [_P, _P, _P, C.c_int32, C.c_float, _P, C.c_int32, _P, _P, C.POINTER(SampleParams),
                                          C.POINTER(RowSampling), C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p,
                                          C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P]),
    "gvc_sample_bias": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                  C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p, C.POINTER(LogitsBias), C.c_int32,
                                  _P, _P]),
    "gvc_gpt_generate_bias": (C.c_int, [_P, _P, _P, C.c_int32, C.c_float, _P, C.c_int32, _P, _P, C.POINTER(SampleParams),
                                        C.POINTER(RowSampling), C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p,
                                        C.POINTER(LogitsBias), C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P,
                                        C.c_int32, C.c_int32, _P]),
    "gvc_sample_ras": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                 C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p, C.POINTER(LogitsBias),
                                 C.POINTER(LogitsRas), _P, C.c_int32, _P, _P]),
    "gvc_gpt_generate_ras": (C.c_int, [_P, _P, _P, C.c_int32, C.c_float, _P, C.c_int32, _P, _P, C.POINTER(SampleParams),
                                       C.POINTER(RowSampling), C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p,
                                       C.POINTER(LogitsBias), C.POINTER(LogitsRas), _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32,
                                       _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P]),
    "gvc_sample_pen": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                 C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p, C.POINTER(LogitsBias),
                                 C.POINTER(LogitsRas), _P, C.POINTER(LogitsPenalties), C.c_int32, _P, _P]),
    "gvc_gpt_generate_pen": (C.c_int, [_P, _P, _P, C.c_int32, C.c_float, _P, C.c_int32, _P, _P, C.POINTER(SampleParams),
                                       C.POINTER(RowSampling), C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p,
                                       C.POINTER(LogitsBias), C.POINTER(LogitsRas), _P, C.POINTER(LogitsPenalties), C.c_int32, C.c_int32,
                                       C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P, C.c_int32, C.c_int32, _P]),
    "gvc_sample_wm": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, _P, C.POINTER(SampleParams), C.POINTER(RowSampling),
                                C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p, C.POINTER(LogitsBias),
                                C.POINTER(LogitsRas), _P, C.POINTER(LogitsPenalties), C.POINTER(LogitsWatermark), C.c_int32, _P, _P]),
    "gvc_gpt_generate_wm": (C.c_int, [_P, _P, _P, C.c_int32, C.c_float, _P, C.c_int32, _P, _P, C.POINTER(SampleParams),
                                      C.POINTER(RowSampling), C.POINTER(LogitsProcessors), C.POINTER(LogitsWarpers), C.c_int32, c_i32p,
                                      C.POINTER(LogitsBias), C.POINTER(LogitsRas), _P, C.POINTER(LogitsPenalties),
                                      C.POINTER(LogitsWatermark), C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32, _P, C.c_int32, _P, _P,
                                      C.c_int32, C.c_int32, _P]),
    "gvc_wm_score": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_transition_scores": (C.c_int, [_P, C.c_int64, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "gvc_gpt_verify": (C.c_int, [_P, _P, C.c_int32, _P, C.c_int32, _P, _P, _P]),
    "gvc_gpt_truncate": (C.c_int, [_P, _P, C.c_int32, _P, _P]),
    "gvc_spec_accept": (C.c_int, [C.POINTER(SpecState), C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, C.POINTER(SampleParams),
                                  C.POINTER(LogitsProcessors), _P]),
    "gvc_gpt_generate_assisted": (C.c_int, [_P, _P, _P, _P, C.POINTER(SpecState), C.POINTER(SampleParams), C.POINTER(LogitsProcessors),
                                            C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P]),
    "gvc_spec_accept_sample": (C.c_int, [C.POINTER(SpecState), C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P,
                                         C.POINTER(SampleParams), C.POINTER(LogitsProcessors), _P]),
    "gvc_gpt_generate_assisted_sample": (C.c_int, [_P, _P, _P, _P, C.POINTER(SpecState), C.POINTER(SpecSampling), C.POINTER(SampleParams),
                                                   C.POINTER(LogitsProcessors), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                   _P]),
    "gvc_spec_lookup": (C.c_int, [C.POINTER(SpecState), C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int32, _P]),
    "gvc_spec_accept_len": (C.c_int, [C.POINTER(SpecState), C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, C.POINTER(SampleParams),
                                      C.POINTER(LogitsProcessors), _P]),
    "gvc_spec_accept_sample_len": (C.c_int, [C.POINTER(SpecState), C.c_int32, C.c_int32, _P, _P, _P, C.c_int32, _P, _P, _P,
                                             C.POINTER(SampleParams), C.POINTER(LogitsProcessors), _P]),
    "gvc_gpt_generate_lookup": (C.c_int, [_P, _P, C.POINTER(SpecState), C.POINTER(SpecSampling), C.POINTER(SampleParams),
                                          C.POINTER(LogitsProcessors), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P,
                                          C.c_int32, _P]),
    "gvc_gpt_decode_variant": (C.c_int, [_P]),
    "gvc_gpt_rows_step_launches": (C.c_longlong, [_P]),
    "gvc_gpt_bf16_gemm_launches": (C.c_longlong, [_P]),
    "gvc_gpt_one_stream_steps": (C.c_longlong, [_P]),
    "gvc_gpt_health": (C.c_int, [_P]),
    "gvc_gpt_warmup": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32]),
    "gvc_gpt_warmup_range": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gvc_gpt_lazy_inits": (C.c_longlong, [_P]),
    "gvc_gpt_rearm": (C.c_int, [_P]),
    "gvc_gpt_time_kernel": (C.c_int, [_P, C.c_int32, _P, C.c_int32, _P, C.c_int32, c_f32p, c_i32p, _P]),
    "gvc_fb16_index": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gvc_gemm_probe": (C.c_int, [C.c_int32, _P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_f32p, _P]),
    "gvc_gemm_probe_ex": (C.c_int, [C.POINTER(GemmCase), _P]),
    "gvc_attn_probe": (C.c_int, [C.POINTER(AttnCase), _P]),
    "gvc_perceiver_create": (C.c_int, [C.POINTER(PerceiverDims), C.POINTER(_P)]),
    "gvc_perceiver_destroy": (C.c_int, [_P]),
    "gvc_perceiver_bind_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "gvc_perceiver_missing_weights": (C.c_int, [_P]),
    "gvc_perceiver_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "gvc_perceiver_forward_masked": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_mel_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32,
                                 c_f32p, C.POINTER(_P)]),
    "gvc_mel_destroy": (C.c_int, [_P]),
    "gvc_mel_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_mel_create_ex": (C.c_int, [C.POINTER(MelOptions), C.POINTER(_P)]),
    "gvc_mel_frames": (C.c_int, [_P, C.c_int32]),
    "gvc_disc_create": (C.c_int, [C.POINTER(DiscDims), C.POINTER(_P)]),
    "gvc_disc_destroy": (C.c_int, [_P]),
    "gvc_disc_bind_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "gvc_disc_missing_weights": (C.c_int, [_P]),
    "gvc_disc_folded_weight": (C.c_int, [_P, C.c_int32, C.c_int32, _P, C.c_int64, _P]),
    "gvc_disc_arena_floats": (C.c_int64, [_P]),
    "gvc_disc_set_arena": (C.c_int, [_P, _P]),
    "gvc_disc_layers": (C.c_int, [_P]),
    "gvc_disc_layer": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), c_i32p, c_i32p, c_i32p]),
    "gvc_disc_forward": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _P, _P]),
    "gvc_disc_time_layer": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, c_f32p, _P]),
    "gvc_l1_mean": (C.c_int, [_P, _P, C.c_int64, C.c_float, _P, _P, _P]),
    "gvc_dvae_create": (C.c_int, [C.POINTER(DvaeDims), C.POINTER(_P)]),
    "gvc_dvae_destroy": (C.c_int, [_P]),
    "gvc_dvae_bind_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "gvc_dvae_missing_weights": (C.c_int, [_P]),
    "gvc_dvae_encode": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_dvae_encode_frames": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_dvae_create_ex": (C.c_int, [C.POINTER(DvaeDims), C.c_int32, C.POINTER(_P)]),
    "gvc_dvae_decode": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_dvae_code_error": (C.c_int, [_P, _P]),
    "gvc_dvae_reconstruct": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P, _P, _P]),
    "gvc_hubert_create": (C.c_int, [C.POINTER(HubertDims), C.POINTER(_P)]),
    "gvc_hubert_destroy": (C.c_int, [_P]),
    "gvc_hubert_bind_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "gvc_hubert_missing_weights": (C.c_int, [_P]),
    "gvc_hubert_frames": (C.c_int, [_P, C.c_int32]),
    "gvc_hubert_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "gvc_hifigan_create": (C.c_int, [C.POINTER(HifiganDims), C.POINTER(_P)]),
    "gvc_hifigan_create_ex": (C.c_int, [C.POINTER(HifiganDimsEx), C.POINTER(_P)]),
    "gvc_hifigan_lds_stages": (C.c_int, [_P]),
    "gvc_hifigan_graph_nodes": (C.c_int, [_P]),
    "gvc_hifigan_destroy": (C.c_int, [_P]),
    "gvc_hifigan_bind_weight": (C.c_int, [_P, C.c_char_p, _P, C.c_int64, _P]),
    "gvc_hifigan_missing_weights": (C.c_int, [_P]),
    "gvc_hifigan_forward": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "gvc_hifigan_forward_latents": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "gvc_resample_length": (C.c_int, [C.c_int32, C.c_int32, C.c_int32]),
    "gvc_resample": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P]),
    "gvc_vq_argmin": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]),
    "gvc_gl_create": (C.c_int, [C.POINTER(GlOptions), c_f32p, C.POINTER(_P)]),
    "gvc_gl_destroy": (C.c_int, [_P]),
    "gvc_gl_inverse_matrix": (C.c_int, [_P, c_f32p]),
    "gvc_gl_inverse_mel": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _P]),
    "gvc_gl_init_angles": (C.c_int, [_P, C.c_uint64, C.c_int32, C.c_int32, _P, _P]),
    "gvc_gl_run": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_float, _P, _P]),
    "gvc_gl_launches": (C.c_longlong, [_P]),
}

_lib = None


GVC_ERR_TIMEOUT = -5          # include/genvc_hip.h: a hand-off of a one-launch step timed out; repeat the call after resetting the slots


class GenvcHipError(RuntimeError):
    """a library call failed; `.code` is its GVC_ERR_* return value (None: raised on the Python side)"""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code

    @property
    def is_handoff_timeout(self):
        return self.code == GVC_ERR_TIMEOUT


def exported_symbols():
    """Names declared in include/genvc_hip.h (used by the CPU test that checks the .so exports them)."""
    return sorted(_SIGNATURES)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GenvcHipError(f"{LIB_PATH} not found: build it with `python -m genvc_amd.build` "
                                "(there is no CPU fallback for the product path)")
        import torch  # noqa: F401  (first: the HIP runtime must be the one torch loads, never two copies)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().gvc_last_error().decode(errors="replace")
        raise GenvcHipError(f"{what} failed with code {rc}: {msg}", rc)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
