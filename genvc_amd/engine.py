"""Thin Python owners of the libgenvc_hip contexts.  torch supplies device memory and the stream;
all arithmetic runs in the HIP library."""
import collections
import ctypes as C
import math

import torch

from . import _lib
from ._lib import check, lib, ptr, stream


def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), "need contiguous fp32 CUDA tensor"
    return t


def _i32(t):
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous(), "need contiguous int32 CUDA tensor"
    return t


def sample_params(sampling, vocab, eos, seed=0):
    return _lib.SampleParams(float(sampling["repetition_penalty"]), float(sampling["temperature"]),
                             float(sampling["top_p"]), int(sampling["top_k"]), int(eos), int(vocab), int(seed))


def row_sampling(rows):
    """rows: an iterable of per-row settings and keys, each a mapping with repetition_penalty, temperature, top_p,
    top_k, seed, rng_row (the row's index inside its job) and rng_step0 (tokens its stream has drawn before this call) ->
    a gvc_row_sampling array (include/genvc_hip.h)"""
    rows = list(rows)
    arr = (_lib.RowSampling * len(rows))()
    for i, r in enumerate(rows):
        arr[i] = _lib.RowSampling(float(r["repetition_penalty"]), float(r["temperature"]), float(r["top_p"]), int(r["top_k"]),
                                  int(r["seed"]), int(r["rng_row"]), int(r["rng_step0"]))
    return arr


def _rows_arg(rows, B):
    arr = rows if isinstance(rows, C.Array) else row_sampling(rows)
    if len(arr) != B:
        raise ValueError(f"{len(arr)} row entries for {B} rows")
    return arr


# HF generate kwargs of the length / repetition processors (include/genvc_hip.h: gvc_logits_processors)
PROC_KWARGS = ("no_repeat_ngram_size", "min_length", "min_new_tokens", "exponential_decay_length_penalty", "suppress_tokens",
               "begin_suppress_tokens", "min_p")
MAX_NGRAM = 8          # GVC_PROC_MAX_NGRAM


def _nonneg_int(kw, name):
    v = kw.get(name)
    if v is None:
        return 0
    if isinstance(v, bool) or int(v) != v or int(v) < 0:
        raise ValueError(f"{name} must be an integer >= 0, not {v!r}")
    return int(v)


def _token_bits(kw, name, vocab):
    toks = kw.get(name)
    if toks is None:
        return [], 0
    toks = [toks] if isinstance(toks, int) else list(toks)
    words = [0] * 33
    for x in toks:
        if isinstance(x, bool) or int(x) != x or not 0 <= int(x) < vocab:
            raise ValueError(f"{name}: token {x!r} outside [0, {vocab})")
        words[int(x) >> 5] |= 1 << (int(x) & 31)
    return words, len(toks)


def logits_processors(kw, prompt_len, vocab, sampling=True, prompt_lens=None):
    """the processor kwargs of one call (PROC_KWARGS, HF semantics) -> a gvc_logits_processors, or None when every one is at its
    default (the kernels then run exactly as without processors).  prompt_len: the prompt length of every row (HF's
    input_ids_seq_length, fake ids included); prompt_lens: a device int32 [B] tensor with one per row instead (kept alive by the
    caller while the call's work runs).  min_p is a warper: it applies only when sampling.  Malformed settings raise ValueError."""
    ngram = _nonneg_int(kw, "no_repeat_ngram_size")
    if ngram > MAX_NGRAM:
        raise ValueError(f"no_repeat_ngram_size {ngram} is above the supported {MAX_NGRAM} (the ban scans the whole row every step)")
    min_length = _nonneg_int(kw, "min_length")
    min_new = _nonneg_int(kw, "min_new_tokens")
    decay = kw.get("exponential_decay_length_penalty")
    start, factor = 0, 0.0
    if decay is not None:
        if not isinstance(decay, (tuple, list)) or len(decay) != 2:
            raise ValueError(f"exponential_decay_length_penalty must be a pair (start, factor), not {decay!r}")
        start, factor = decay
        if isinstance(start, bool) or int(start) != start:
            raise ValueError(f"exponential_decay_length_penalty start must be an integer, not {start!r}")
        if not float(factor) > 0.0:
            raise ValueError(f"exponential_decay_length_penalty factor must be > 0, not {factor!r}")
        start, factor = int(start), float(factor)
    min_p = kw.get("min_p")
    min_p = 0.0 if min_p is None else float(min_p)
    if not 0.0 <= min_p <= 1.0:
        raise ValueError(f"min_p must be in [0, 1], not {min_p!r}")
    if not sampling:
        min_p = 0.0
    sup, n_sup = _token_bits(kw, "suppress_tokens", vocab)
    bsup, n_bsup = _token_bits(kw, "begin_suppress_tokens", vocab)
    if not (ngram or min_length or min_new or factor or min_p or n_sup or n_bsup):
        return None
    pr = _lib.LogitsProcessors()
    pr.no_repeat_ngram_size, pr.min_length, pr.min_new_tokens, pr.decay_start = ngram, min_length, min_new, start
    pr.decay_factor, pr.min_p, pr.prompt_len = factor, min_p, int(prompt_len)
    pr.n_suppress, pr.n_begin_suppress = n_sup, n_bsup
    if prompt_lens is not None:
        pr.prompt_lens = _i32(prompt_lens).data_ptr()
    for i in range(33):
        pr.suppress[i] = sup[i] if n_sup else 0
        pr.begin_suppress[i] = bsup[i] if n_bsup else 0
    return pr


MAX_SET_ROWS = 64      # kMaxSampleRows: rows of a call with per-row processor sets


# HF generate kwargs of the entropy-aware sampling warpers (include/genvc_hip.h: gvc_logits_warpers), applied after min_p
WARP_KWARGS = ("typical_p", "epsilon_cutoff", "eta_cutoff")


def _warp_value(kw, name):
    v = kw.get(name)
    if v is None:
        return None
    if isinstance(v, bool):
        raise ValueError(f"{name} must be a number, not {v!r}")
    try:
        return float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, not {v!r}") from None


def logits_warpers(kw, sampling=True):
    """the warper kwargs of one call (WARP_KWARGS) -> a gvc_logits_warpers, or None when every one is off or `sampling` is False (the
    call then passes no warpers at all).  On / off follow transformers' _get_logits_processor: typical_p < 1 builds the warper, which
    raises ValueError for typical_p <= 0; epsilon_cutoff and eta_cutoff act inside (0, 1) and are silently off outside it; with
    do_sample=False none is built."""
    typ, eps, eta = (_warp_value(kw, k) for k in WARP_KWARGS)
    if not sampling:
        return None
    w = _lib.LogitsWarpers()
    if typ is not None and typ < 1.0:
        if not typ > 0.0:
            raise ValueError(f"`typical_p` has to be a float > 0 and < 1, but is {typ}")
        w.typical_p = typ
    if eps is not None and 0.0 < eps < 1.0:
        w.epsilon_cutoff = eps
    if eta is not None and 0.0 < eta < 1.0:
        w.eta_cutoff = eta
    # an on value that rounds to 0 or 1 in float32 (0 is "off" on the device, 1 is out of range) stays just inside (0, 1)
    for f, v in zip(WARP_KWARGS, (typ, eps, eta)):
        if getattr(w, f) >= 1.0:
            setattr(w, f, 1.0 - 2.0 ** -24)
        elif getattr(w, f) == 0.0 and v is not None and 0.0 < v < 1.0:
            setattr(w, f, 2.0 ** -126)
    if not (w.typical_p or w.epsilon_cutoff or w.eta_cutoff):
        return None
    return w


# generation kwargs of repetition-aware sampling (include/genvc_hip.h: gvc_logits_ras): not HF's, the codec-LM decoders'
RAS_KWARGS = ("ras_window", "ras_threshold")
RAS_MAX_WINDOW = _lib.RAS_MAX_WINDOW
RAS_DEFAULT_THRESHOLD = 0.1


def ras_counts(kw):
    """the RAS_KWARGS of one call -> (window K, min_count), or None when RAS is off (ras_window None or 0).
    min_count = max(1, ceil(ras_threshold * K - 1e-9)): the device compares integers only.  ValueError: a window that is no integer
    in 0..64 (a bool is none), a threshold outside (0, 1] or no number, a threshold without a window."""
    K, tau = kw.get("ras_window"), kw.get("ras_threshold")
    if K is not None and (isinstance(K, bool) or not isinstance(K, int)):
        raise ValueError(f"ras_window must be an integer in 0..{RAS_MAX_WINDOW} (0 or None: off), not {K!r}")
    if K is not None and not 0 <= K <= RAS_MAX_WINDOW:
        raise ValueError(f"ras_window must be in 0..{RAS_MAX_WINDOW} (0 or None: off), not {K!r}")
    if tau is not None and (isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0.0 < float(tau) <= 1.0):
        raise ValueError(f"ras_threshold must be a number in (0, 1], not {tau!r}")
    if not K:
        if tau is not None:
            raise ValueError(f"ras_threshold={tau!r} without ras_window: the threshold is a share of the window")
        return None
    tau = RAS_DEFAULT_THRESHOLD if tau is None else float(tau)
    return int(K), max(1, math.ceil(tau * K - 1e-9))


def logits_ras(kw, prompt_len):
    """the RAS_KWARGS of one call -> a gvc_logits_ras, or None when RAS is off (the call then passes no table at all).
    prompt_len: the prompt length of the rows (fake ids included), the one min_new_tokens counts from: only ids behind it are
    generated tokens.  Malformed settings raise ValueError (ras_counts)."""
    kc = ras_counts(kw)
    if kc is None:
        return None
    r = _lib.LogitsRas()
    r.window, r.min_count = kc
    r.prompt_len = int(prompt_len)
    return r


class RasTable:
    """the RAS entries of one call beside its sets (include/genvc_hip.h: gvc_gpt_generate_ras): `ras` holds one gvc_logits_ras per
    entry of the call's ProcessorSets / WarperSets (window 0 where the entry has none), or one entry for every row of a call without
    sets; `redraws` is the int32 [B] device counter of the rows (or None), which the caller zeroes."""

    def __init__(self, entries, redraws=None):
        self.n = len(entries)
        self.ras = (_lib.LogitsRas * self.n)(*[_lib.LogitsRas() if r is None else r for r in entries])
        self.redraws = redraws


# generation kwargs of the presence / frequency / windowed repetition penalties (include/genvc_hip.h: gvc_logits_penalties; DESIGN.md
# 4.29): the OpenAI / vLLM definition of the first two, and a window of recent generated tokens for all three penalties
PENALTY_KWARGS = ("presence_penalty", "frequency_penalty", "penalty_window")
PENALTY_MAX = _lib.PENALTY_MAX


def penalty_settings(kw):
    """the PENALTY_KWARGS of one call -> (presence, frequency, window), or None when all are off (each None or 0).
    ValueError: a presence / frequency that is no finite number in [-2, 2] (a bool is none), a window that is no integer >= 0."""
    vals = []
    for k in PENALTY_KWARGS[:2]:
        v = kw.get(k)
        if v is None:
            vals.append(0.0)
            continue
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not -PENALTY_MAX <= v <= PENALTY_MAX:
            raise ValueError(f"{k} must be a finite number in [-{PENALTY_MAX:g}, {PENALTY_MAX:g}] (0 or None: off), not {v!r}")
        vals.append(float(v))
    W = kw.get("penalty_window")
    if W is not None and (isinstance(W, bool) or not isinstance(W, int) or W < 0 or W > 0x7fffffff):
        raise ValueError(f"penalty_window must be an integer >= 0 (0 or None: every generated token), not {W!r}")
    W = int(W or 0)
    if vals[0] == 0.0 and vals[1] == 0.0 and W == 0:
        return None
    return vals[0], vals[1], W


def logits_penalties(kw, prompt_len):
    """the PENALTY_KWARGS of one call -> a gvc_logits_penalties, or None when they are off (the call then passes no table at all).
    prompt_len: the prompt length of the rows (fake ids included): only ids behind it are generated tokens.  Malformed settings raise
    ValueError (penalty_settings)."""
    pfw = penalty_settings(kw)
    if pfw is None:
        return None
    q = _lib.LogitsPenalties()
    q.presence, q.frequency, q.window = pfw
    q.prompt_len = int(prompt_len)
    return q


class PenaltyTable:
    """the penalty entries of one call beside its sets (include/genvc_hip.h: gvc_gpt_generate_pen): one gvc_logits_penalties per entry
    of the call's ProcessorSets / WarperSets (all-zero where the entry has none), or one entry for every row of a call without sets"""

    def __init__(self, entries):
        self.n = len(entries)
        self.pen = (_lib.LogitsPenalties * self.n)(*[_lib.LogitsPenalties() if q is None else q for q in entries])


# The green-list watermark (Kirchenbauer et al.; transformers' `watermarking_config` of generate and its WatermarkDetector; include/
# genvc_hip.h: gvc_logits_watermark).  The kwarg is HF's; its value a dict with HF's keys, or an object with to_dict().
# key -> table is DEFINED by the CPU torch.Generator (a CUDA generator gives other permutations): what this produces, and what the
# detector accepts, is what transformers' processor / detector built with device="cpu" produce and accept.
WATERMARK_KWARGS = ("watermarking_config",)
WATERMARK_KEYS = ("greenlist_ratio", "bias", "hashing_key", "seeding_scheme", "context_width")
WATERMARK_SCHEMES = {"lefthash": _lib.WM_LEFTHASH, "selfhash": _lib.WM_SELFHASH}
MAX_WATERMARK_TABLES = 8          # device-resident tables of one GptEngine
WatermarkSettings = collections.namedtuple("WatermarkSettings", WATERMARK_KEYS)
_WM_DEFAULTS = dict(greenlist_ratio=0.25, bias=2.0, hashing_key=15485863, seeding_scheme="lefthash", context_width=1)
_WM_FIXED_TABLE = 1_000_003       # transformers' table_size of the selfhash scheme
_wm_tables = {}                   # (key, ratio, scheme, V) -> the host table, built once per process


def watermark_settings(kw, vocab):
    """kw["watermarking_config"] of one call -> WatermarkSettings, or None when it is absent or None (off: the call passes no table).
    ValueError: a value that is neither a dict nor has to_dict(), an unknown key, an unknown seeding_scheme, a greenlist_ratio outside
    (0, 1) or so small that int(vocab * ratio) == 0, a non-finite bias, a hashing_key that is no integer in [0, 2**63), a bool anywhere.
    NotImplementedError: context_width != 1 (lefthash: the width changes nothing in generation; selfhash: width 2 needs vocab ** 2
    permutations on the host)."""
    cfg = (kw or {}).get("watermarking_config")
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        if isinstance(cfg, bool) or not callable(getattr(cfg, "to_dict", None)):
            raise ValueError(f"watermarking_config must be a dict, an object with to_dict() or None, not {cfg!r}")
        cfg = cfg.to_dict()
    unknown = sorted(set(cfg) - set(WATERMARK_KEYS), key=str)
    if unknown:
        raise ValueError(f"watermarking_config: {unknown[0]!r} is not one of its keys ({', '.join(WATERMARK_KEYS)})")
    v = dict(_WM_DEFAULTS, **{k: x for k, x in cfg.items() if x is not None})
    for k, x in v.items():
        if isinstance(x, bool):
            raise ValueError(f"watermarking_config: {k} must not be a bool ({x!r})")
    if v["seeding_scheme"] not in WATERMARK_SCHEMES:
        raise ValueError(f"watermarking_config: seeding_scheme has to be one of ['selfhash', 'lefthash'], not {v['seeding_scheme']!r}")
    r = v["greenlist_ratio"]
    if not isinstance(r, (int, float)) or not 0.0 < r < 1.0:          # (a NaN fails both comparisons)
        raise ValueError(f"watermarking_config: greenlist_ratio has to lie between 0.0 and 1.0, exclusively, not {r!r}")
    if int(vocab * r) == 0:
        raise ValueError(f"watermarking_config: greenlist_ratio {r!r} leaves no green id among {vocab}")
    if not isinstance(v["bias"], (int, float)) or not math.isfinite(v["bias"]):
        raise ValueError(f"watermarking_config: bias must be a finite number, not {v['bias']!r}")
    key = v["hashing_key"]
    if not isinstance(key, int) or not 0 <= key < 2 ** 63:
        raise ValueError(f"watermarking_config: hashing_key must be an integer in [0, 2**63), not {key!r}")
    w = v["context_width"]
    if not isinstance(w, int):
        raise ValueError(f"watermarking_config: context_width must be an integer, not {w!r}")
    if w != 1:
        raise NotImplementedError(f"watermarking_config: context_width={w} is not implemented (1 is): the green list of a step is a "
                                  "table row chosen by the previous code alone")
    return WatermarkSettings(float(r), float(v["bias"]), int(key), v["seeding_scheme"], 1)


def watermark_table(settings, vocab):
    """WatermarkSettings -> the green lists as a uint32 [rows, ceil(vocab / 32)] CPU tensor: bit (i & 31) of word (i >> 5) of row
    `prev` is set when id i is green after prev (lefthash: vocab rows); selfhash: ONE row, the ids that are green after themselves.
    Built as transformers' WatermarkLogitsProcessor(vocab, "cpu", ...) builds its lists: a CPU torch.Generator seeded with
    (hashing_key * prev) % (2**64 - 1) (lefthash) or with the wrapped int64 product hashing_key * a * a, a = fixed_table[cand] + 1
    (selfhash, fixed_table = randperm(1_000_003) under the key), and the first int(vocab * ratio) ids of randperm(vocab).  Cached per
    (key, ratio, scheme, vocab) in the process; the tensor is shared: do not write to it."""
    import numpy as np
    ck = (settings.hashing_key, settings.greenlist_ratio, settings.seeding_scheme, int(vocab))
    if ck in _wm_tables:
        return _wm_tables[ck]
    V = int(vocab)
    words = (V + 31) // 32
    n_green = int(V * settings.greenlist_ratio)
    g = torch.Generator(device="cpu")
    key = settings.hashing_key
    selfhash = settings.seeding_scheme == "selfhash"
    if selfhash:
        g.manual_seed(key)
        fixed = torch.randperm(_WM_FIXED_TABLE, generator=g, device="cpu")
        ab = fixed[torch.arange(V) % _WM_FIXED_TABLE] + 1
        seeds = [int(s) % (2 ** 64 - 1) for s in (key * ab * ab).tolist()]          # int64 tensor arithmetic: it wraps, as HF's does
    else:
        seeds = [(key * prev) % (2 ** 64 - 1) for prev in range(V)]
    bits = np.zeros((1 if selfhash else V, words * 32), dtype=bool)
    for c, seed in enumerate(seeds):
        g.manual_seed(seed)
        green = torch.randperm(V, generator=g, device="cpu")[:n_green].numpy()
        if selfhash:
            bits[0, c] = bool((green == c).any())
        else:
            bits[c, green] = True
    packed = np.packbits(bits.reshape(bits.shape[0], words, 32), axis=-1, bitorder="little").view("<u4").reshape(bits.shape[0], words)
    t = torch.from_numpy(np.ascontiguousarray(packed.astype(np.uint32)))
    _wm_tables[ck] = t
    return t


class WatermarkTable:
    """the watermark entries of one call beside its sets (include/genvc_hip.h: gvc_gpt_generate_wm): one gvc_logits_watermark per
    entry of the call's ProcessorSets / WarperSets (a null table where the entry has none), or one entry for every row of a call
    without sets.  entries: what GptEngine.watermark_entry() returned (or None).  The tables are slots of the engine's arena; this
    object holds them (GptEngine.watermark_release on release() or when it is collected), so no other call can rewrite a slot while a
    loop that reads it is alive."""

    def __init__(self, entries, engine=None):
        self.n = len(entries)
        self.wm = (_lib.LogitsWatermark * self.n)(*[_lib.LogitsWatermark() if m is None else m[0] for m in entries])
        self._engine = engine
        self._held = [m[1] for m in entries if m is not None and m[1] is not None]

    def release(self):
        held, self._held = self._held, []
        if self._engine is not None:
            for k in held:
                self._engine.watermark_release(k)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class WatermarkDetector:
    """transformers' WatermarkDetector for code sequences, the counts on the device (include/genvc_hip.h: gvc_wm_score).
    watermarking_config: as the generation kwarg (dict / to_dict() object); vocab: the code vocabulary the mark was made with;
    ignore_repeated_ngrams: count each distinct (prev, cur) pair -- each distinct code under selfhash -- once, at its first occurrence.
    The tables are those of a CPU generator (watermark_table): this detects what this project marks and what an HF processor built
    with device="cpu" marks, not the output of an HF processor on a CUDA generator.
    __call__(codes [B, n] or [n] integer tensor (moved to the GPU if it is not there), lens=None ([B] valid lengths), z_threshold=3.0,
    return_dict=False) -> the boolean predictions (numpy [B]), or with return_dict a dict of num_tokens_scored, num_green_tokens,
    green_fraction, z_score, p_value, prediction, confidence (numpy, float64 where HF's are; HF's formulas on the host) and `flags`
    (uint8 [B, n] CPU tensor: 1 green, 0 scored and not green, 2 unscored).  lefthash scores len - 1 codes of a row, selfhash len; an
    id outside [0, vocab) makes its n-gram unscored.  A row with nothing scored has z = nan and prediction False.  n <= 8192."""

    def __init__(self, watermarking_config, vocab, ignore_repeated_ngrams=False):
        s = watermark_settings(dict(watermarking_config=watermarking_config), vocab)
        if s is None:
            raise ValueError("WatermarkDetector needs a watermarking_config (None detects nothing)")
        self.settings, self.vocab, self.ignore_repeated_ngrams = s, int(vocab), bool(ignore_repeated_ngrams)
        self._host = watermark_table(s, vocab)
        self._dev = {}          # device -> the table there

    def counts(self, codes, lens=None):
        """-> (counts int32 [B, 2] (scored, green), flags uint8 [B, n]), both on the device"""
        if codes.ndim == 1:
            codes = codes[None]
        if codes.ndim != 2 or codes.is_floating_point() or codes.shape[1] < 1 or codes.shape[0] < 1:
            raise ValueError(f"WatermarkDetector: codes must be an integer tensor [B, n] with B, n >= 1, not {tuple(codes.shape)} {codes.dtype}")
        if codes.shape[1] > _lib.WM_MAX_SCORE_LEN:
            raise ValueError(f"WatermarkDetector: {codes.shape[1]} codes per row, at most {_lib.WM_MAX_SCORE_LEN}")
        if not codes.is_cuda:
            codes = codes.cuda()
        dev = codes.device
        codes = codes.to(torch.int32).contiguous()
        B, n = codes.shape
        if lens is not None:
            lens = torch.as_tensor(lens, device=dev).to(torch.int32).contiguous()
            if tuple(lens.shape) != (B,):
                raise ValueError(f"WatermarkDetector: lens {tuple(lens.shape)} for {B} rows")
        if dev not in self._dev:
            self._dev[dev] = self._host.view(torch.int32).to(dev)
        table = self._dev[dev]
        counts = torch.empty(B, 2, device=dev, dtype=torch.int32)
        flags = torch.empty(B, n, device=dev, dtype=torch.uint8)
        check(lib().gvc_wm_score(ptr(codes), None if lens is None else ptr(lens), B, n, ptr(table),
                                 WATERMARK_SCHEMES[self.settings.seeding_scheme], int(self._host.shape[1]), self.vocab,
                                 int(self.ignore_repeated_ngrams), ptr(counts), ptr(flags), stream()), "wm_score")
        return counts, flags

    def __call__(self, codes, lens=None, z_threshold=3.0, return_dict=False):
        counts, flags = self.counts(codes, lens)
        out = watermark_statistics(counts.cpu().numpy(), self.settings.greenlist_ratio, z_threshold)
        if not return_dict:
            return out["prediction"]
        out["flags"] = flags.cpu()
        return out


def watermark_statistics(counts, greenlist_ratio, z_threshold=3.0):
    """counts [B, 2] (scored, green) -> transformers' WatermarkDetectorOutput fields as a dict of numpy arrays, float64 with HF's
    formulas: z = (green - r * scored) / sqrt(scored * r * (1 - r)), p = 1 - 0.5 * (1 + sign(z) * (1 - exp(-2 z^2 / pi)))"""
    import numpy as np
    c = np.asarray(counts)
    scored, green = c[:, 0].astype(np.float64), c[:, 1].astype(np.float64)
    r = greenlist_ratio
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (green - r * scored) / np.sqrt(scored * r * (1 - r))
        p = 1 - (0.5 * (1 + np.sign(z) * (1 - np.exp(-2 * z ** 2 / np.pi))))
        frac = green / scored
    return dict(num_tokens_scored=scored, num_green_tokens=green, green_fraction=frac, z_score=z, p_value=p, prediction=z > z_threshold,
                confidence=1 - p)


# HF generate kwargs of the call-wide sequence bias / bad words / forced EOS / renormalised scores (include/genvc_hip.h: gvc_logits_bias)
BIAS_KWARGS = ("sequence_bias", "bad_words_ids", "forced_eos_token_id", "forced_bos_token_id", "renormalize_logits")
BIAS_MAX_SEQS = _lib.BIAS_MAX_SEQS      # entries of sequence_bias and bad_words_ids together
BIAS_MAX_LEN = _lib.BIAS_MAX_LEN        # ids of one entry


def _bias_ids(name, seq, vocab):
    """one id sequence of sequence_bias / bad_words_ids -> a tuple of ints in [0, vocab), 1..BIAS_MAX_LEN of them"""
    if isinstance(seq, (str, bytes)) or not hasattr(seq, "__iter__"):
        raise ValueError(f"{name}: an entry must be a sequence of token ids, not {seq!r}")
    seq = tuple(seq)
    if not 1 <= len(seq) <= BIAS_MAX_LEN:
        raise ValueError(f"{name}: an entry holds {len(seq)} ids; the device matches 1..{BIAS_MAX_LEN}")
    for x in seq:
        if isinstance(x, bool) or int(x) != x or not 0 <= int(x) < vocab:
            raise ValueError(f"{name}: token {x!r} outside [0, {vocab})")
    return tuple(int(x) for x in seq)


def _sequence_bias(value, vocab):
    """sequence_bias in either HF form -- {tuple(ids): float} or [[ids, float], ...] -> [(ids, float)] in HF's order of application:
    the length-1 entries, then the longer ones in dict order (the list form becomes a dict first, as in HF: a repeated sequence keeps
    its first place and its last value)"""
    if value is None:
        return []
    if isinstance(value, dict):
        items = list(value.items())
    elif isinstance(value, (list, tuple)):
        items = []
        for e in value:
            if not isinstance(e, (list, tuple)) or len(e) != 2:
                raise ValueError(f"sequence_bias: a list entry must be [ids, bias], not {e!r}")
            items.append((e[0], e[1]))
    else:
        raise ValueError(f"sequence_bias must be a dict {{tuple(ids): float}} or a list [[ids, float], ...], not {type(value).__name__}")
    merged = {}
    for seq, v in items:
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise ValueError(f"sequence_bias: the bias of {seq!r} must be a number, not {v!r}")
        v = float(v)
        if v != v or v == float("inf"):
            raise ValueError(f"sequence_bias: the bias of {seq!r} must be finite or -inf, not {v!r}")
        merged[_bias_ids("sequence_bias", seq, vocab)] = v
    out = [(k, v) for k, v in merged.items() if len(k) == 1]
    return out + [(k, v) for k, v in merged.items() if len(k) > 1]


def logits_bias(kw, prompt_len, max_new, vocab, eos):
    """the BIAS_KWARGS of one call (HF semantics, transformers 5.x SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor /
    ForcedEOSTokenLogitsProcessor / LogitNormalization) -> a gvc_logits_bias, or None when every one is off: None, {} / [], False, and
    bad_words_ids == [[eos]] (HF drops a bare [eos]).  prompt_len: the prompt length of every row (fake ids included); max_new: the
    call's max_new_tokens (the forced EOS fires at the step that writes token max_new - 1).  Ids lie in [0, vocab) in both forms of
    sequence_bias (HF's list form refuses 0: the one deviation).  forced_eos_token_id must be `eos` -- the loop knows one stop token --
    and the stop token must not be suppressed with it (the row would be all -inf).  forced_bos_token_id is accepted and does nothing:
    HF's processor fires at cur_len == 1, and no prompt of this model is that short.  Malformed settings raise ValueError."""
    seqs = _sequence_bias(kw.get("sequence_bias"), vocab)
    bad = kw.get("bad_words_ids")
    bans = []
    if bad is not None:
        if isinstance(bad, (str, bytes, dict)) or not hasattr(bad, "__iter__"):
            raise ValueError(f"bad_words_ids must be a list of lists of token ids, not {bad!r}")
        for seq in bad:
            ids = _bias_ids("bad_words_ids", seq, vocab)
            if ids != (int(eos),) and ids not in bans:
                bans.append(ids)
    if len(seqs) + len(bans) > BIAS_MAX_SEQS:
        raise ValueError(f"sequence_bias ({len(seqs)}) and bad_words_ids ({len(bans)}) hold {len(seqs) + len(bans)} entries together; the "
                         f"device matches {BIAS_MAX_SEQS} per step")
    force = kw.get("forced_eos_token_id")
    if force is not None:
        if isinstance(force, (list, tuple)) and len(force) == 1:
            force = force[0]
        if isinstance(force, bool) or not isinstance(force, int) or force != int(eos):
            raise ValueError(f"forced_eos_token_id={kw.get('forced_eos_token_id')!r} must be the model's stop token {int(eos)}: the "
                             "generation loop knows one EOS")
        sup = list(kw.get("suppress_tokens") or ())
        if int(max_new) == 1:
            sup += list(kw.get("begin_suppress_tokens") or ())
        if int(eos) in [int(x) for x in sup]:
            raise ValueError(f"forced_eos_token_id={int(eos)} with the stop token suppressed leaves the last step no token at all")
        if int(max_new) < 1:
            raise ValueError(f"forced_eos_token_id needs max_new_tokens >= 1, not {max_new}")
    bos = kw.get("forced_bos_token_id")
    if bos is not None and (isinstance(bos, bool) or not isinstance(bos, int) or not 0 <= bos < vocab):
        raise ValueError(f"forced_bos_token_id: token {bos!r} outside [0, {vocab})")
    renorm = kw.get("renormalize_logits")
    if renorm is not None and not isinstance(renorm, bool):
        raise ValueError(f"renormalize_logits must be a bool, not {renorm!r}")
    if not (seqs or bans or force is not None or renorm):
        return None
    z = _lib.LogitsBias()
    z.n_bias, z.n_ban = len(seqs), len(bans)
    z.force_eos_at = int(max_new) if force is not None else 0
    z.renormalize = 1 if renorm else 0
    z.prompt_len = int(prompt_len)
    for e, (ids, v) in enumerate(seqs + [(b, float("-inf")) for b in bans]):
        z.len[e] = len(ids)
        z.bias[e] = v
        for q, x in enumerate(ids):
            z.ids[e][q] = x
    return z


def check_proc_kwargs(kw, where):
    """a per-row / per-group / per-job / per-session processor dict may hold PROC_KWARGS, WARP_KWARGS, RAS_KWARGS, PENALTY_KWARGS and
    WATERMARK_KWARGS only: anything else raises ValueError naming the key and `where` it came from"""
    if kw is None:
        return
    if not isinstance(kw, dict):
        raise ValueError(f"{where}: processor kwargs must be a dict or None, not {type(kw).__name__}")
    allowed = PROC_KWARGS + WARP_KWARGS + RAS_KWARGS + PENALTY_KWARGS + WATERMARK_KWARGS
    unknown = sorted(set(kw) - set(allowed))
    if unknown:
        raise ValueError(f"{where}: {unknown[0]!r} is not a processor kwarg (allowed: {', '.join(allowed)})")


def _kw_key(kw):
    """hashable form of a processor dict (lists become tuples), for de-duplication before packing"""
    key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()
                       if v is not None and k not in WATERMARK_KWARGS))          # (the mark is no part of a processor set)
    try:
        hash(key)
    except TypeError:           # (an array-like value: its repr still tells identical dicts apart)
        key = repr(key)
    return key


class ProcessorSets:
    """per-row processor sets of one call (include/genvc_hip.h: gvc_gpt_generate_proc_sets): `sets` (n_sets gvc_logits_processors) and
    `set_of_row` (B int32 indices into them, -1 = no processors), both host arrays.  `prompt_lens` keeps the caller's device tensor
    alive (the sets point at it)."""

    def __init__(self, sets, set_of_row, prompt_lens=None):
        self.n_sets = len(sets)
        self.sets = (_lib.LogitsProcessors * self.n_sets)(*sets)
        self.set_of_row = (C.c_int32 * len(set_of_row))(*set_of_row)
        self.prompt_lens = prompt_lens

    def __len__(self):
        return len(self.set_of_row)


def logits_processor_sets(kws, prompt_len, vocab, sampling=True, prompt_lens=None):
    """per-row processor kwargs -> ProcessorSets, or None when no row has a processor (the call then passes no sets at all).
    kws: one entry per row, a dict of PROC_KWARGS (validated as logits_processors() does) or None for a row without processors.
    prompt_len: the prompt length of every row (int) or of each row (a sequence of B ints: rows with equal dicts and different prompts
    then get sets of their own); prompt_lens: a device int32 [B] tensor with one per row instead, as in logits_processors().
    Identical dicts, and dicts that pack to the same set, share one set.  Errors name the offending row."""
    kws = list(kws)
    B = len(kws)
    if not 1 <= B <= MAX_SET_ROWS:
        raise ValueError(f"per-row processor sets serve 1..{MAX_SET_ROWS} rows, not {B}")
    plens = [prompt_len] * B if isinstance(prompt_len, int) else [int(x) for x in prompt_len]
    if len(plens) != B:
        raise ValueError(f"{len(plens)} prompt lengths for {B} rows")
    if prompt_lens is not None:
        if int(prompt_lens.numel()) != B:
            raise ValueError(f"{int(prompt_lens.numel())} prompt lengths for {B} rows")
        plens = [0] * B
    by_kw, by_bytes, sets, index = {}, {}, [], []
    for b, kw in enumerate(kws):
        check_proc_kwargs(kw, f"row {b}")
        if not kw:
            index.append(-1)
            continue
        key = (_kw_key(kw), plens[b])
        if key not in by_kw:
            try:
                pr = logits_processors(kw, plens[b], vocab, sampling=sampling, prompt_lens=prompt_lens)
            except ValueError as e:
                raise ValueError(f"row {b}: {e}") from None
            if pr is None:
                by_kw[key] = -1
            else:
                raw = C.string_at(C.addressof(pr), C.sizeof(pr))
                if raw not in by_bytes:
                    by_bytes[raw] = len(sets)
                    sets.append(pr)
                by_kw[key] = by_bytes[raw]
        index.append(by_kw[key])
    if not sets:
        return None
    return ProcessorSets(sets, index, prompt_lens)


class WarperSets:
    """per-row processor sets with warpers (include/genvc_hip.h: gvc_gpt_generate_warp): n_sets entries, each a gvc_logits_processors
    (`sets` is None when no entry has one; an entry without one is the all-zero struct) paired with a gvc_logits_warpers, and
    `set_of_row` (B int32 indices, -1 = neither), all host arrays.  `prompt_lens` keeps the caller's device tensor alive.
    `ras` (optional): a gvc_logits_ras or None per entry; with any set, `self.ras` is the call's RasTable (generate_call passes it on).
    `pen` (optional): a gvc_logits_penalties or None per entry; with any set, `self.pen` is the call's PenaltyTable likewise.
    `wm` (optional): what `engine`.watermark_entry() returned, or None, per entry; with any set, `self.wm` is the call's
    WatermarkTable likewise (it holds the entries' table slots while this object lives)."""

    def __init__(self, procs, warps, set_of_row, prompt_lens=None, ras=None, pen=None, wm=None, engine=None):
        self.n_sets = len(warps)
        self.wm = WatermarkTable(list(wm), engine) if wm is not None and any(m is not None for m in wm) else None
        self.pen = PenaltyTable(list(pen)) if pen is not None and any(q is not None for q in pen) else None
        self.ras = RasTable(list(ras)) if ras is not None and any(r is not None for r in ras) else None
        self.sets = None
        if any(p is not None for p in procs):
            self.sets = (_lib.LogitsProcessors * self.n_sets)(*[_lib.LogitsProcessors() if p is None else p for p in procs])
        self.warps = (_lib.LogitsWarpers * self.n_sets)(*[_lib.LogitsWarpers() if w is None else w for w in warps])
        self.set_of_row = (C.c_int32 * len(set_of_row))(*set_of_row)
        self.prompt_lens = prompt_lens

    @classmethod
    def one(cls, proc, warp, B):
        """one call-wide entry (proc may be None) for all B rows"""
        if not 1 <= B <= MAX_SET_ROWS:
            raise ValueError(f"the sampling warpers serve calls of 1..{MAX_SET_ROWS} rows, not {B}")
        return cls([proc], [warp], [0] * B)

    def __len__(self):
        return len(self.set_of_row)


def logits_sets(kws, prompt_len, vocab, sampling=True, prompt_lens=None, engine=None):
    """logits_processor_sets() whose per-row dicts may also hold WARP_KWARGS, RAS_KWARGS, PENALTY_KWARGS and WATERMARK_KWARGS.  When
    no row has a warper, RAS, a penalty or a watermark on, this returns exactly what logits_processor_sets() returns (a ProcessorSets
    or None); otherwise a WarperSets, rows with equal processors, warpers, RAS, penalty and watermark entries (settings and prompt
    length) sharing an entry.  A row with watermarking_config needs `engine`, the GptEngine whose arena holds the tables: rows with
    different keys get entries of their own, pointing at different slots.  Errors name the offending row."""
    kws = list(kws)
    ps = logits_processor_sets(kws, prompt_len, vocab, sampling=sampling, prompt_lens=prompt_lens)      # (validates every row)
    plens = [prompt_len] * len(kws) if isinstance(prompt_len, int) else [int(x) for x in prompt_len]
    warps, rass, pens, wms = [], [], [], []
    for b, kw in enumerate(kws):
        try:
            warps.append(logits_warpers(kw or {}, sampling))
            rass.append(logits_ras(kw or {}, plens[b]))
            pens.append(logits_penalties(kw or {}, plens[b]))
            wms.append(watermark_settings(kw or {}, vocab))
        except ValueError as e:
            raise ValueError(f"row {b}: {e}") from None
    if all(w is None for w in warps) and all(r is None for r in rass) and all(q is None for q in pens) and all(m is None for m in wms):
        return ps
    if engine is None and any(m is not None for m in wms):
        raise ValueError("watermarking_config in a per-row dict needs the engine whose arena holds the tables: logits_sets(engine=...)")
    if prompt_lens is not None and any(r is not None for r in rass):
        raise ValueError("ras_window counts a row's generated tokens from a host prompt length: pass prompt_len, not a device tensor")
    if prompt_lens is not None and any(q is not None for q in pens):
        raise ValueError("the presence / frequency / windowed penalties count a row's generated tokens from a host prompt length: pass "
                         "prompt_len, not a device tensor")
    pidx = list(ps.set_of_row) if ps is not None else [-1] * len(kws)
    by, procs, wl, rl, ql, ml, index = {}, [], [], [], [], [], []

    def raw(x):
        return None if x is None else C.string_at(C.addressof(x), C.sizeof(x))
    for b, (w, r, q, m) in enumerate(zip(warps, rass, pens, wms)):
        if pidx[b] < 0 and w is None and r is None and q is None and m is None:
            index.append(-1)
            continue
        key = (pidx[b], raw(w), raw(r), raw(q), m)
        if key not in by:
            by[key] = len(wl)
            procs.append(ps.sets[pidx[b]] if pidx[b] >= 0 else None)
            wl.append(w)
            rl.append(r)
            ql.append(q)
            ml.append(None if m is None else engine.watermark_entry(m))
        index.append(by[key])
    return WarperSets(procs, wl, index, prompt_lens, ras=rl, pen=ql, wm=ml, engine=engine)


BEAM_LENGTH_MODES = {"4.33": 0, "generated": 1}


def beam_early_stopping(value):
    """HF's early_stopping (False, True or "never") -> the device's code (gvc_beam_state, bits 8..15 of length_mode)"""
    for v, code in ((False, 0), (True, 1), ("never", 2)):
        if value is v or (isinstance(v, str) and value == v):
            return code
    raise ValueError(f"early_stopping must be a boolean or 'never', but is {value!r}")


class BeamSearch:
    """device state of one deterministic beam search (gvc_beam_state, include/genvc_hip.h) over B items of K beams: double-buffered
    ids rows, running scores, the finished-hypothesis store, the copy lists of the last reorder.  `fake` [B, n0] are the fake ids of
    compute_embeddings (every beam of an item starts from them).  early_stopping: False, True or "never" (the item-done test of
    k_beam_select)."""

    def __init__(self, fake, K, max_new, eos, vocab, length_penalty=1.0, repetition_penalty=1.0, length_mode="4.33", proc=None,
                 early_stopping=False):
        if length_mode not in BEAM_LENGTH_MODES:
            raise ValueError(f"beam_length_mode must be one of {sorted(BEAM_LENGTH_MODES)}, not {length_mode!r}")
        dev = fake.device
        B, n0 = fake.shape
        self.B, self.K, self.n0, self.max_new, self.eos = B, K, n0, max_new, eos
        W = n0 + max_new + 8
        i32 = dict(device=dev, dtype=torch.int32)
        self.ids = torch.full((2, B * K, W), eos, **i32)
        self.ids[0, :, :n0] = fake.to(torch.int32).repeat_interleave(K, 0)
        self.scores = torch.zeros(B, K, device=dev, dtype=torch.float32)
        self.scores[:, 1:] = -1e9
        self.scores = self.scores.reshape(-1).contiguous()
        self.tokens = torch.zeros(B * K, **i32)
        self.parents = torch.zeros(B * K, **i32)
        self.done = torch.zeros(B, **i32)
        self.hyp_score = torch.zeros(B, K, device=dev, dtype=torch.float32)
        self.hyp_len = torch.zeros(B, K, **i32)
        self.hyp_tok = torch.full((B, K, max_new), eos, **i32)
        self.hyp_count = torch.zeros(B, **i32)
        self.hyp_worst = torch.full((B,), 1e9, device=dev, dtype=torch.float32)
        self.copies = torch.zeros(B, K, 3, **i32)
        self.n_copies = torch.zeros(B, **i32)
        self.steps = 0
        self.early_stopping = early_stopping
        self.c = _lib.BeamState(B, K, int(vocab), int(eos), n0, W, int(max_new),
                                BEAM_LENGTH_MODES[length_mode] | (beam_early_stopping(early_stopping) << 8), float(length_penalty),
                                float(repetition_penalty), *[t.data_ptr() for t in (
                                    self.ids, self.scores, self.tokens, self.parents, self.done, self.hyp_score, self.hyp_len,
                                    self.hyp_tok, self.hyp_count, self.hyp_worst, self.copies, self.n_copies)])
        self.length_mode = length_mode
        self.length_penalty = float(length_penalty)
        self.proc = proc          # gvc_logits_processors (logits_processors()) or None

    def finalize(self, num_return=1):
        """BeamSearchScorer.finalize: the running beams of the items not done join their hypotheses (length n0 + T in mode "4.33", T
        in mode "generated"), the num_return best hypotheses per item win, best first at rows b * num_return + j; rows are their
        tokens, then eos (= pad) up to the longest returned row + 1 (at most max_new).  Returns (ids int64 [B * num_return, n], their
        scores [B * num_return]); once per call, host-side torch on the device"""
        B, K, T = self.B, self.K, self.steps
        N = int(num_return)
        if not 1 <= N <= K:
            raise ValueError(f"`num_return_sequences` ({N}) has to be smaller or equal to `num_beams` ({K}), and at least 1")
        L = self.n0 + T if BEAM_LENGTH_MODES[self.length_mode] == 0 else T
        ids = self.ids[T & 1].view(B, K, -1)[:, :, self.n0:self.n0 + T]
        done = self.done.bool().cpu()
        cnt = self.hyp_count.cpu()
        hs, hl = self.hyp_score.cpu(), self.hyp_len.cpu()
        run = (self.scores.view(B, K) / (float(L) ** self.length_penalty)).cpu()
        best = []
        for b in range(B):
            items = [(float(hs[b, i]), ("h", i)) for i in range(int(cnt[b]))]
            if not done[b]:
                # (BeamHypotheses.add in beam order, so the kept set is the one the reference keeps)
                for k in range(K):
                    sc = float(run[b, k])
                    if len(items) < K:
                        items.append((sc, ("r", k)))
                    elif sc > min(s for s, _ in items):
                        del items[min(range(len(items)), key=lambda i: (items[i][0], i))]
                        items.append((sc, ("r", k)))
            best.extend((b, it) for it in sorted(items, key=lambda x: x[0])[::-1][:N])      # (sorted_hyps.pop(): the best first)
        rows = []
        for b, (sc, (kind, i)) in best:
            rows.append(self.hyp_tok[b, i, :int(hl[b, i])] if kind == "h" else ids[b, i])
        width = min(max(int(r.shape[0]) for r in rows) + 1, self.max_new)
        out = torch.full((B * N, width), self.eos, device=self.ids.device, dtype=torch.long)
        for b, r in enumerate(rows):
            n = min(int(r.shape[0]), width)
            out[b, :n] = r[:n].long()
        return out, torch.tensor([sc for _, (sc, _) in best], dtype=torch.float64)


def beam_select(beam, logits, slots, t):
    """one select step of `beam` (a BeamSearch) on logits [B*K, vocab] at step t; slots [B*K] int32 are permuted in place
    (include/genvc_hip.h: gvc_beam_select)"""
    if beam.proc is None:
        check(lib().gvc_beam_select(C.byref(beam.c), ptr(_f32(logits)), ptr(_i32(slots)), int(t), stream()), "beam_select")
    else:
        check(lib().gvc_beam_select_proc(C.byref(beam.c), C.byref(beam.proc), ptr(_f32(logits)), ptr(_i32(slots)), int(t), stream()),
              "beam_select_proc")


def check_beam_groups(K, G, diversity_penalty):
    """HF's rules for num_beams = K, num_beam_groups = G, diversity_penalty (ValueError each): G in [1, K], K % G == 0, a finite
    diversity_penalty >= 0 that is positive only with G > 1 (plain beam search has no Hamming processor to hand it to)"""
    K, G, lam = int(K), int(G), float(diversity_penalty)
    if G < 1:
        raise ValueError(f"`num_beam_groups` has to be an integer strictly greater than 0, but is {G}")
    if G > K:
        raise ValueError(f"`num_beam_groups` ({G}) has to be smaller or equal to `num_beams` ({K})")
    if K % G != 0:
        raise ValueError(f"`num_beams` ({K}) should be divisible by `num_beam_groups` ({G}) for group beam search")
    if lam != lam or lam in (float("inf"), float("-inf")) or lam < 0.0:
        raise ValueError(f"`diversity_penalty` has to be a finite float >= 0, but is {diversity_penalty!r}")
    if lam > 0.0 and G == 1:
        raise ValueError(f"`diversity_penalty` ({lam}) is not 0.0 but `num_beam_groups` is 1: it only has an effect in group beam search")
    return K, G, lam


class GroupBeamSearch(BeamSearch):
    """device state of one group (diverse) beam search (gvc_beam_state + gvc_beam_groups, include/genvc_hip.h): BeamSearch's arrays
    with the K rows of an item read as G groups of S = K / G (rows g*S .. g*S + S-1), the running score 0 at the first beam of every
    group, and the per-(item, group) done flags, hypothesis counts and worst kept scores.  G == 1 is the plain search."""

    def __init__(self, fake, K, G, diversity_penalty, max_new, eos, vocab, length_penalty=1.0, repetition_penalty=1.0, length_mode="4.33",
                 proc=None, early_stopping=False):
        K, G, lam = check_beam_groups(K, G, diversity_penalty)
        super().__init__(fake, K, max_new, eos, vocab, length_penalty, repetition_penalty, length_mode, proc, early_stopping)
        B, dev = self.B, fake.device
        self.G, self.S, self.diversity_penalty = G, K // G, lam
        self.scores.view(B, K)[:, ::self.S] = 0.0
        self.group_done = torch.zeros(B, G, device=dev, dtype=torch.int32)
        self.group_count = torch.zeros(B, G, device=dev, dtype=torch.int32)
        self.group_worst = torch.full((B, G), 1e9, device=dev, dtype=torch.float32)
        self.g = _lib.BeamGroups(G, lam, self.group_done.data_ptr(), self.group_count.data_ptr(), self.group_worst.data_ptr())

    def finalize(self, num_return=1):
        """BeamSearchScorer.finalize with num_beam_groups: the running beams of every group not done join that group's set (capacity
        S, in beam order), the num_return best hypotheses over the G sets of an item win, best first at rows b * num_return + j (a
        stable descending sort over the sets in group order, each in its kept order).  Returns as BeamSearch.finalize"""
        B, K, G, S, T = self.B, self.K, self.G, self.S, self.steps
        N = int(num_return)
        if not 1 <= N <= K:
            raise ValueError(f"`num_return_sequences` ({N}) has to be smaller or equal to `num_beams` ({K}), and at least 1")
        L = self.n0 + T if BEAM_LENGTH_MODES[self.length_mode] == 0 else T
        ids = self.ids[T & 1].view(B, K, -1)[:, :, self.n0:self.n0 + T]
        done = self.group_done.bool().cpu()
        cnt = self.group_count.cpu()
        hs, hl = self.hyp_score.cpu(), self.hyp_len.cpu()
        run = (self.scores.view(B, K) / (float(L) ** self.length_penalty)).cpu()
        best = []
        for b in range(B):
            cand = []
            for g in range(G):
                items = [(float(hs[b, g * S + i]), ("h", g * S + i)) for i in range(int(cnt[b, g]))]
                if not done[b, g]:
                    for k in range(g * S, (g + 1) * S):
                        sc = float(run[b, k])
                        if len(items) < S:
                            items.append((sc, ("r", k)))
                        elif sc > min(s for s, _ in items):
                            del items[min(range(len(items)), key=lambda i: (items[i][0], i))]
                            items.append((sc, ("r", k)))
                cand.extend(items)
            best.extend((b, it) for it in sorted(cand, key=lambda x: x[0])[::-1][:N])
        rows = []
        for b, (sc, (kind, i)) in best:
            rows.append(self.hyp_tok[b, i, :int(hl[b, i])] if kind == "h" else ids[b, i])
        width = min(max(int(r.shape[0]) for r in rows) + 1, self.max_new)
        out = torch.full((B * N, width), self.eos, device=self.ids.device, dtype=torch.long)
        for b, r in enumerate(rows):
            n = min(int(r.shape[0]), width)
            out[b, :n] = r[:n].long()
        return out, torch.tensor([sc for _, (sc, _) in best], dtype=torch.float64)


def group_beam_select(beam, logits, slots, t):
    """one select step of `beam` (a GroupBeamSearch) on logits [B*K, vocab] at step t, the groups walked in order inside one launch;
    slots [B*K] int32 are permuted in place, group by group (include/genvc_hip.h: gvc_group_beam_select)"""
    check(lib().gvc_group_beam_select(C.byref(beam.c), C.byref(beam.g), C.byref(beam.proc) if beam.proc is not None else None,
                                      ptr(_f32(logits)), ptr(_i32(slots)), int(t), stream()), "group_beam_select")


MAX_CONTRASTIVE_K = 16    # kCsMaxK (csrc/contrastive.h)


class ContrastiveSearch:
    """device state of one contrastive search (gvc_contrastive_state, include/genvc_hip.h) over B items of K candidates: the ids rows,
    finished flags, tokens and latents, and the prompt's hidden rows [B, n0, d] that the prefill writes (GptEngine.prefill_hidden).
    `fake` [B, n0] are the fake ids of compute_embeddings."""

    def __init__(self, fake, K, max_new, eos, vocab, d, penalty_alpha, repetition_penalty=1.0, proc=None, latents=True):
        dev = fake.device
        B, n0 = fake.shape
        self.B, self.K, self.n0, self.max_new, self.eos = B, K, n0, max_new, eos
        W = n0 + max_new + 8
        i32 = dict(device=dev, dtype=torch.int32)
        self.ids = torch.full((B, W), eos, **i32)
        self.ids[:, :n0] = fake.to(torch.int32)
        self.finished = torch.zeros(B, **i32)
        self.tokens = torch.full((B, max_new), eos, **i32)
        self.latents = torch.empty(B, max_new, d, device=dev, dtype=torch.float32) if latents else None
        self.hidden0 = torch.empty(B, n0, d, device=dev, dtype=torch.float32)
        self.steps = 0
        self.c = _lib.ContrastiveState(B, K, int(vocab), int(eos), n0, W, int(max_new), float(penalty_alpha), float(repetition_penalty), 0,
                                       self.ids.data_ptr(), self.finished.data_ptr(), self.tokens.data_ptr(),
                                       self.latents.data_ptr() if latents else None, self.hidden0.data_ptr())
        self.proc = proc          # gvc_logits_processors (logits_processors()) or None


MAX_ASSISTANT_TOKENS = 15    # kSpecMaxDrafts (csrc/spec.h): drafts per round of an assisted generation
MAX_VERIFY_ROWS = 128        # kSpecMaxRows: rows of one verification pass, B * (k + 1)
MAX_LOOKUP_NGRAM = 8         # kSpecMaxNgram: the longest suffix a prompt lookup searches for
MAX_LOOKUP_HISTORY = 2048    # kSpecMaxHistory: ids of one row's history a prompt lookup stages (the ids row behind `from`)


class AssistedState:
    """device-side state of one assisted (speculative) greedy generation over B streams (include/genvc_hip.h: gvc_spec_state): the
    ids rows, per-row lengths, emitted counts, finished flags and pending tokens, the result buffers, the counters and the workspace
    of the rounds.  `fake` int [B, n0]: the prompt's fake ids; k: drafts per round"""

    def __init__(self, fake, k, max_new, eos, vocab, d, latents=True):
        B, n0 = fake.shape
        dev = fake.device
        if isinstance(k, bool) or int(k) != k or not 0 <= int(k) <= MAX_ASSISTANT_TOKENS:
            raise ValueError(f"an assisted round drafts 0..{MAX_ASSISTANT_TOKENS} tokens, not {k!r}")
        k = int(k)
        if B * (k + 1) > MAX_VERIFY_ROWS:
            raise ValueError(f"{B} streams x {k + 1} rows exceed the {MAX_VERIFY_ROWS} rows of one verification pass")

        def i32(*shape, fill=0):
            return torch.full(shape, fill, device=dev, dtype=torch.int32)
        self.B, self.k, self.n0, self.max_new, self.eos, self.vocab, self.d = B, k, n0, int(max_new), int(eos), int(vocab), int(d)
        self.ids = i32(B, n0 + self.max_new + MAX_ASSISTANT_TOKENS + 1)
        self.ids[:, :n0] = fake.to(torch.int32)
        self.ids_len = i32(B, fill=n0)
        self.finished, self.emitted, self.pending = i32(B), i32(B), i32(B, fill=-1)
        self.toks = i32(B, self.max_new, fill=self.eos)
        self.lats = torch.zeros(B, self.max_new, self.d, device=dev, dtype=torch.float32) if latents else None
        self.drop_target, self.drop_assistant = i32(B), i32(B)
        self.rounds, self.drafted, self.accepted = i32(B), i32(B), i32(B)
        self.v_toks = i32(B, MAX_ASSISTANT_TOKENS + 1)
        self.v_logits = torch.zeros(B, MAX_ASSISTANT_TOKENS + 1, self.vocab, device=dev, dtype=torch.float32)
        self.v_latents = torch.zeros(B, MAX_ASSISTANT_TOKENS + 1, self.d, device=dev, dtype=torch.float32)
        self.d_ids_len, self.d_finished = i32(B), i32(B)
        self.draft_len = i32(B)      # drafts per row of a prompt-lookup round (gvc_spec_lookup writes it, the accept step reads it)
        self.opened = False          # the opening step (token 0 from the prefill's parked logits) has run
        self.rounds_done = 0         # rounds enqueued so far (every live row emits at least one token per round)
        p = (lambda t: None if t is None else t.data_ptr())
        self.c = _lib.SpecState(B, self.ids.shape[1], self.max_new, self.toks.stride(0), self.max_new, self.d, p(self.ids),
                                p(self.ids_len), p(self.finished), p(self.emitted), p(self.pending), p(self.toks), p(self.lats),
                                p(self.drop_target), p(self.drop_assistant), p(self.rounds), p(self.drafted), p(self.accepted),
                                p(self.v_toks), p(self.v_logits), p(self.v_latents), p(self.d_ids_len), p(self.d_finished))

    def sampling(self):
        """the workspaces of speculative sampling (include/genvc_hip.h: gvc_spec_sampling), allocated on first use: the draft's and
        the target's warped rows fp32 [B, 16, V] and the draft sampler's keyed rows (32 bytes per stream)"""
        if getattr(self, "_sampling", None) is None:
            dev = self.ids.device
            self.q_scores = torch.zeros(self.B, MAX_ASSISTANT_TOKENS + 1, self.vocab, device=dev, dtype=torch.float32)
            self.p_scores = torch.zeros(self.B, MAX_ASSISTANT_TOKENS + 1, self.vocab, device=dev, dtype=torch.float32)
            self.key_rows = torch.zeros(self.B, C.sizeof(_lib.RowSampling), device=dev, dtype=torch.uint8)
            self._sampling = _lib.SpecSampling(self.q_scores.data_ptr(), self.p_scores.data_ptr(), self.key_rows.data_ptr())
        return self._sampling

    def stats(self):
        """the device counters as int64 [B] tensors: rounds run, drafts compared and drafts accepted per row"""
        return dict(rounds=self.rounds.long(), drafted=self.drafted.long(), accepted=self.accepted.long())


def spec_lookup(state, k, max_ngram, start, q_scores=None):
    """the prompt lookup of one round on `state` (include/genvc_hip.h: gvc_spec_lookup): k drafts per row from the longest suffix (up
    to max_ngram ids) of ids[start .. ids_len) that occurs earlier in it.  Fills state.v_toks (as [B, k + 1]) and state.draft_len;
    q_scores fp32 [B, k + 1, V] (optional) gets the drafts' one-hot rows as warped scores (0 at the token, -inf elsewhere)"""
    assert q_scores is None or (tuple(q_scores.shape) == (state.B, k + 1, state.vocab) and q_scores.is_contiguous())
    check(lib().gvc_spec_lookup(C.byref(state.c), int(k), int(max_ngram), int(start), ptr(state.draft_len),
                                ptr(None if q_scores is None else _f32(q_scores)), state.vocab, stream()), "spec_lookup")


def spec_accept(state, k, appended, logits, latents, drafts, params, proc=None, draft_len=None):
    """the accept step of an assisted round on `state` (include/genvc_hip.h: gvc_spec_accept): logits fp32 [B, k + 1, V], latents fp32
    [B, k + 1, d] or None, drafts int32 [B, >= k] or None for k = 0; appended: rows both caches gained (k + 1, or 0 for an opening step).
    draft_len int32 [B] (optional; gvc_spec_accept_len): the drafts each row has, fewer than k where its source found fewer"""
    B = state.B
    assert tuple(logits.shape) == (B, k + 1, state.vocab) and (latents is None or tuple(latents.shape) == (B, k + 1, state.d))
    if draft_len is not None:
        assert tuple(draft_len.shape) == (B,)
        check(lib().gvc_spec_accept_len(C.byref(state.c), int(k), int(appended), ptr(_f32(logits)),
                                        ptr(None if latents is None else _f32(latents)), ptr(None if drafts is None else _i32(drafts)),
                                        0 if drafts is None else drafts.shape[1], ptr(_i32(draft_len)), C.byref(params),
                                        None if proc is None else C.byref(proc), stream()), "spec_accept_len")
        return
    check(lib().gvc_spec_accept(C.byref(state.c), int(k), int(appended), ptr(_f32(logits)), ptr(None if latents is None else _f32(latents)),
                                ptr(None if drafts is None else _i32(drafts)), 0 if drafts is None else drafts.shape[1], C.byref(params),
                                None if proc is None else C.byref(proc), stream()), "spec_accept")


def spec_accept_sample(state, k, appended, logits, latents, drafts, q_scores, params, proc=None, draft_len=None):
    """the accept step of speculative sampling on `state`, warping included (include/genvc_hip.h: gvc_spec_accept_sample): arguments as
    spec_accept, plus q_scores fp32 [B, k + 1, V] (row j: the warped row draft j was drawn from; None for k = 0) and every sampling
    field of `params`.  Returns the target's warped rows fp32 [B, k + 1, V] (rows the step did not need are left as they were).
    draft_len int32 [B] (optional; gvc_spec_accept_sample_len): as in spec_accept"""
    B = state.B
    assert tuple(logits.shape) == (B, k + 1, state.vocab) and (latents is None or tuple(latents.shape) == (B, k + 1, state.d))
    assert q_scores is None or tuple(q_scores.shape) == (B, k + 1, state.vocab)
    p_rows = torch.zeros(B, k + 1, state.vocab, device=logits.device, dtype=torch.float32)
    if draft_len is not None:
        assert tuple(draft_len.shape) == (B,)
        check(lib().gvc_spec_accept_sample_len(C.byref(state.c), int(k), int(appended), ptr(_f32(logits)),
                                               ptr(None if latents is None else _f32(latents)),
                                               ptr(None if drafts is None else _i32(drafts)), 0 if drafts is None else drafts.shape[1],
                                               ptr(_i32(draft_len)), ptr(None if q_scores is None else _f32(q_scores)), ptr(p_rows),
                                               C.byref(params), None if proc is None else C.byref(proc), stream()),
              "spec_accept_sample_len")
        return p_rows
    check(lib().gvc_spec_accept_sample(C.byref(state.c), int(k), int(appended), ptr(_f32(logits)),
                                       ptr(None if latents is None else _f32(latents)), ptr(None if drafts is None else _i32(drafts)),
                                       0 if drafts is None else drafts.shape[1], ptr(None if q_scores is None else _f32(q_scores)),
                                       ptr(p_rows), C.byref(params), None if proc is None else C.byref(proc), stream()),
          "spec_accept_sample")
    return p_rows


# host names of gvc_gpt_dims.weight_dtype (include/genvc_hip.h)
WEIGHT_DTYPES = {"fp32": 0, "bf16": 1, "bf16_kv": 2, "bf16_act": 3, "bf16_mfma": 4}


class GptEngine:
    """KV-cached GPT-2 stack of GenVC (reference layers/gpt.py + layers/gpt_inference.py)."""

    def __init__(self, dims, max_slots=8, max_rows=2048, max_seq=None, weight_dtype="fp32"):
        self.dims = dict(dims)
        self.d = dims["d_model"]
        self.V = dims["num_audio_tokens"]
        self.max_slots = max_slots
        self.max_rows = max_rows
        self.weight_dtype = weight_dtype
        max_seq = max_seq or ((dims["max_seq"] + 63) // 64) * 64
        cd = _lib.GptDims(dims["n_layer"], dims["d_model"], dims["n_head"], dims["num_audio_tokens"],
                          dims["max_mel_pos"], dims["max_text_pos"], dims["number_text_tokens"], max_seq,
                          max_slots, max_rows, WEIGHT_DTYPES[weight_dtype])
        self._h = C.c_void_p()
        self._pending_side = None     # end-of-work event of another stream of this process (watch_stream)
        self.side_joins = 0
        check(lib().gvc_gpt_create(C.byref(cd), C.byref(self._h)), "gvc_gpt_create")

    def close(self):
        if self._h:
            lib().gvc_gpt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, weights, prefix=""):
        """weights: name -> CUDA fp32 tensor, named as the reference GPT state dict."""
        for name, t in weights.items():
            if not name.startswith(prefix) or not torch.is_tensor(t) or not t.is_floating_point():
                continue
            t = _f32(t.detach().to(torch.float32).contiguous())
            check(lib().gvc_gpt_bind_weight(self._h, name[len(prefix):].encode(), ptr(t), t.numel(), stream()),
                  f"bind {name}")
        torch.cuda.current_stream().synchronize()      # sources may be temporaries
        missing = lib().gvc_gpt_missing_weights(self._h)
        if missing:
            raise _lib.GenvcHipError(f"{missing} GPT weight tensors missing after bind")

    def prefix_embeddings(self, cond_latents, codes):
        B, n_cond, _ = cond_latents.shape
        Tc = codes.shape[1]
        out = torch.empty(B, n_cond + Tc + 2, self.d, device=cond_latents.device, dtype=torch.float32)
        check(lib().gvc_gpt_prefix_embeddings(self._h, ptr(_f32(cond_latents)), n_cond, ptr(_i32(codes)), B, Tc,
                                              self.dims["start_text_token"], self.dims["stop_text_token"],
                                              ptr(out), stream()), "prefix_embeddings")
        return out

    def watch_stream(self, event):
        """Residency before issue: the one-launch steps need all 256 workgroups co-resident, so work of this process that is still in
        flight on ANOTHER stream (the conditioning side stream of model_init._CondFuture: mel + Perceiver, ~25 short launches) must not
        overlap them -- a missing workgroup costs a ~0.2 s bounded spin and a fallback (include/genvc_hip.h: gvc_gpt_health).  The owner of
        such a stream registers the event that marks the end of its work here; the next prefill / decode_step / generate / latents call
        makes the caller's stream wait for it first (`side_joins` counts the calls that really had to wait)."""
        self._pending_side = event

    def _join_side(self):
        ev = self._pending_side
        if ev is not None:
            self._pending_side = None
            if not ev.query():
                torch.cuda.current_stream().wait_event(ev)
                self.side_joins += 1

    def prefill(self, slots, prefix_emb, want_outputs=True, n_cached=0):
        """n_cached > 0: the first n_cached rows of the prefix (the conditioning latents) are already in the slots' KV
        cache from an earlier prefill with the same leading rows -- only the rest is computed (bit-identical results)"""
        self._join_side()
        B, P, _ = prefix_emb.shape
        logits = latent = None
        if want_outputs:
            logits = torch.empty(B, self.V, device=prefix_emb.device, dtype=torch.float32)
            latent = torch.empty(B, self.d, device=prefix_emb.device, dtype=torch.float32)
        check(lib().gvc_gpt_prefill_cached(self._h, ptr(_i32(slots)), B, ptr(_f32(prefix_emb)), P, int(n_cached),
                                           self.dims["start_audio_token"], ptr(logits), ptr(latent), stream()), "prefill")
        return logits, latent

    def prefill_cond(self, slots, cond_latents):
        """the conditioning rows alone into the slots' KV caches (include/genvc_hip.h: gvc_gpt_prefill_cond): later prefills of these slots
        pass n_cached = cond_latents.shape[1]"""
        self._join_side()
        B, n, _ = cond_latents.shape
        check(lib().gvc_gpt_prefill_cond(self._h, ptr(_i32(slots)), B, ptr(_f32(cond_latents)), n, stream()), "prefill_cond")

    def decode_step(self, slots, tok, logits=None, latent=None):
        self._join_side()
        B = slots.shape[0]
        if logits is None:
            logits = torch.empty(B, self.V, device=slots.device, dtype=torch.float32)
            latent = torch.empty(B, self.d, device=slots.device, dtype=torch.float32)
        check(lib().gvc_gpt_decode_step(self._h, ptr(_i32(slots)), B, ptr(_i32(tok)), ptr(logits), ptr(latent),
                                        stream()), "decode_step")
        return logits, latent

    def reset(self, slots):
        check(lib().gvc_gpt_reset_slots(self._h, ptr(_i32(slots)), slots.shape[0], stream()), "reset_slots")

    def kv_fanout(self, src_slots, dst_slots):
        """slot src_slots[i] -> slot dst_slots[i] (int32 device tensors of equal length): the cached K/V rows, the length / mel position
        and the parked logits / latent, so the destination continues as the source would (include/genvc_hip.h: gvc_gpt_kv_fanout)"""
        self._join_side()
        n = int(src_slots.shape[0])
        if int(dst_slots.shape[0]) != n:
            raise ValueError(f"kv_fanout: {n} source slots for {int(dst_slots.shape[0])} destinations")
        check(lib().gvc_gpt_kv_fanout(self._h, ptr(_i32(src_slots)), ptr(_i32(dst_slots)), n, stream()), "kv_fanout")

    def sequence_logprobs(self, tokens, latents, token_logprobs=False):
        """tokens int32 [R, >= n], latents fp32 [R, n, d] (a generation loop's latents_out) -> (logprob [R] float64, length [R] int32):
        the summed log-probability of each row's tokens up to and including its first stop token, under the raw model distribution
        (include/genvc_hip.h: gvc_gpt_sequence_logprobs).  token_logprobs=True: also the per-token terms [R, n] fp32"""
        self._join_side()
        latents = _f32(latents.contiguous())
        tokens = _i32(tokens.contiguous())
        R, n, d = latents.shape
        if d != self.d or tokens.shape[0] != R or tokens.shape[1] < n or n < 1:
            raise ValueError(f"sequence_logprobs: tokens {tuple(tokens.shape)} do not go with latents {tuple(latents.shape)} "
                             f"(d_model {self.d})")
        lp = torch.empty(R, device=latents.device, dtype=torch.float64)
        ln = torch.empty(R, device=latents.device, dtype=torch.int32)
        tl = torch.empty(R, n, device=latents.device, dtype=torch.float32) if token_logprobs else None
        check(lib().gvc_gpt_sequence_logprobs(self._h, ptr(tokens), tokens.stride(0), ptr(latents), R, n, self.dims["stop_audio_token"],
                                              ptr(lp), ptr(ln), ptr(tl), stream()), "sequence_logprobs")
        return (lp, ln, tl) if token_logprobs else (lp, ln)

    def latents(self, slots, prefix_emb, gen_codes):
        self._join_side()
        B, P, _ = prefix_emb.shape
        n = gen_codes.shape[1]
        out = torch.empty(B, n, self.d, device=prefix_emb.device, dtype=torch.float32)
        check(lib().gvc_gpt_latents(self._h, ptr(_i32(slots)), B, ptr(_f32(prefix_emb)), P, ptr(_i32(gen_codes)), n,
                                    self.dims["start_audio_token"], self.dims["stop_audio_token"], ptr(out),
                                    stream()), "latents")
        return out

    def trace(self, slots, prefix_emb, gen_codes, lengths, n_cond, output_attentions=True, output_hidden_states=False, alignment=True,
              alignment_layers=None):
        """the trace pass (include/genvc_hip.h: gvc_gpt_trace) over prefix_emb fp32 [B, P, d] (of prefix_embeddings: n_cond conditioning
        rows, text start, Tc content codes, text stop) and gen_codes int32 [B, n] with generated lengths `lengths` [B] (stop code counted)
        -> (probs fp32 [L, B, H, T, T] or None, hidden fp32 [L + 1, B, T, d] or None, align fp32 [B, n, Tc] or None), T = P + n.
        alignment_layers: the layers the alignment averages over (indices, negative from the end; None = all)."""
        self._join_side()
        prefix_emb, gen_codes = _f32(prefix_emb.contiguous()), _i32(gen_codes.contiguous())
        B, P, _ = prefix_emb.shape
        n = int(gen_codes.shape[1])
        T, L, H = P + n, self.dims["n_layer"], self.dims["n_head"]
        Tc = P - int(n_cond) - 2
        if gen_codes.shape[0] != B or slots.shape[0] != B or Tc < 1:
            raise ValueError(f"trace: prefix {tuple(prefix_emb.shape)} ({n_cond} conditioning rows), codes {tuple(gen_codes.shape)} and "
                             f"{int(slots.shape[0])} slots do not go together")
        lens_host = torch.as_tensor(lengths).to("cpu", torch.int32).contiguous()
        if tuple(lens_host.shape) != (B,):
            raise ValueError(f"trace: {tuple(lens_host.shape)} lengths for {B} items")
        mask = 0
        if alignment_layers is not None:
            for l in alignment_layers:
                if not -L <= int(l) < L:
                    raise ValueError(f"trace: alignment layer {l} outside the model's {L} layers")
                mask |= 1 << (int(l) % L)
            if mask == 0:
                raise ValueError("trace: alignment_layers is empty")
        dev = prefix_emb.device
        lens_dev = lens_host.to(dev)
        probs = torch.empty(L, B, H, T, T, device=dev, dtype=torch.float32) if output_attentions else None
        hidden = torch.empty(L + 1, B, T, self.d, device=dev, dtype=torch.float32) if output_hidden_states else None
        align = torch.empty(B, n, Tc, device=dev, dtype=torch.float32) if alignment else None
        scratch = torch.empty(B, H, T, T, device=dev, dtype=torch.float32) if alignment and probs is None else None
        opt = _lib.TraceOptions(start_tok=self.dims["start_audio_token"], stop_tok=self.dims["stop_audio_token"], content_off=int(n_cond) + 1,
                                n_content=Tc, layer_mask=mask, probs=None if probs is None else probs.data_ptr(),
                                hidden=None if hidden is None else hidden.data_ptr(), align=None if align is None else align.data_ptr(),
                                scratch=None if scratch is None else scratch.data_ptr())
        rc = lib().gvc_gpt_trace(self._h, ptr(_i32(slots)), B, ptr(prefix_emb), P, ptr(gen_codes), n, ptr(lens_dev),
                                 C.c_void_p(lens_host.data_ptr()), C.byref(opt), stream())
        if rc == -4:
            raise NotImplementedError(f"trace: attentions and hidden states come from a reference-numerics pass -- this context was created "
                                      f"with weight_dtype=\"{self.weight_dtype}\" ({lib().gvc_last_error().decode(errors='replace')})")
        if rc == -1:
            raise ValueError(f"trace: {lib().gvc_last_error().decode(errors='replace')}")
        check(rc, "trace")
        return probs, hidden, align

    def _eval_check(self, rc, what):
        """status of an evaluation-pass entry: argument errors as ValueError, a bf16 context as NotImplementedError naming its mode"""
        if rc == -4:
            raise NotImplementedError(f"{what}: the evaluation pass runs in reference numerics only -- this context was created with "
                                      f"weight_dtype=\"{self.weight_dtype}\" ({lib().gvc_last_error().decode(errors='replace')})")
        if rc == -1:
            raise ValueError(f"{what}: {lib().gvc_last_error().decode(errors='replace')}")
        check(rc, what)

    def forward_rows(self, slots, cond_latents, text_ids, code_ids, key_mask=None):
        """cond_latents fp32 [B, n_cond, d], text_ids int32 [B, Lt], code_ids int32 [B, Lm], key_mask uint8 / bool [B, n_cond + Lt + Lm]
        (nonzero = attend; None: no mask) -> final_norm(ln_f(h)) of the Lt + Lm rows behind the conditioning ones, fp32 [B, Lt + Lm, d]
        (include/genvc_hip.h: gvc_gpt_forward_rows)"""
        self._join_side()
        cond_latents = _f32(cond_latents.contiguous())
        text_ids, code_ids = _i32(text_ids.contiguous()), _i32(code_ids.contiguous())
        B, n_cond, d = cond_latents.shape
        Lt, Lm = int(text_ids.shape[1]), int(code_ids.shape[1])
        if d != self.d or text_ids.shape[0] != B or code_ids.shape[0] != B or slots.shape[0] != B:
            raise ValueError(f"forward_rows: cond {tuple(cond_latents.shape)}, text ids {tuple(text_ids.shape)}, code ids "
                             f"{tuple(code_ids.shape)} and {int(slots.shape[0])} slots do not go together (d_model {self.d})")
        if key_mask is not None:
            if tuple(key_mask.shape) != (B, n_cond + Lt + Lm):
                raise ValueError(f"forward_rows: key mask {tuple(key_mask.shape)} for {B} x {n_cond + Lt + Lm} rows")
            key_mask = key_mask.to(torch.uint8).contiguous()
        out = torch.empty(B, Lt + Lm, self.d, device=cond_latents.device, dtype=torch.float32)
        self._eval_check(lib().gvc_gpt_forward_rows(self._h, ptr(_i32(slots)), B, ptr(cond_latents), n_cond, ptr(text_ids), Lt,
                                                    ptr(code_ids), Lm, ptr(key_mask), ptr(out), stream()), "forward_rows")
        return out

    def head_xent(self, latents, head, targets, label_smoothing=0.0, top_k=10):
        """latents fp32 [R, d], head "text" / "mel", targets int32 [R] (-1 = ignored) -> (logits fp32 [R, V], row_terms fp32 [R, 3] =
        (nll, smoothing term, top-k hit), sums float64 [4] = (loss, hits, count, mean nll))   (include/genvc_hip.h: gvc_gpt_head_xent)"""
        latents = _f32(latents.contiguous())
        targets = _i32(targets.contiguous())
        R = int(latents.shape[0])
        if latents.ndim != 2 or latents.shape[1] != self.d or tuple(targets.shape) != (R,):
            raise ValueError(f"head_xent: latents {tuple(latents.shape)} / targets {tuple(targets.shape)} (d_model {self.d})")
        V = {"text": self.dims["number_text_tokens"], "mel": self.V}[head]
        logits = torch.empty(R, V, device=latents.device, dtype=torch.float32)
        terms = torch.empty(R, 3, device=latents.device, dtype=torch.float32)
        sums = torch.empty(4, device=latents.device, dtype=torch.float64)
        self._eval_check(lib().gvc_gpt_head_xent(self._h, ptr(latents), R, 1 if head == "mel" else 0, ptr(targets), float(label_smoothing),
                                                 int(top_k), ptr(logits), ptr(terms), ptr(sums), stream()), "head_xent")
        return logits, terms, sums

    # ---- the sampler and generation entry points: families of C entries (include/genvc_hip.h), one marshalling path each ----------------
    def _neutral_params(self):
        """the common params of a call whose rows carry their own settings: eos and vocab, everything else neutral"""
        return sample_params(dict(repetition_penalty=1.0, temperature=1.0, top_p=1.0, top_k=0), self.V, self.dims["stop_audio_token"])

    def _lat_stride(self, tokens_out, latents_out):
        """checks the output buffers of a generation call -> the row stride of latents_out in rows of d (0 without latents)"""
        assert tokens_out.is_cuda and tokens_out.dtype == torch.int32 and tokens_out.stride(1) == 1
        if latents_out is None:
            return 0
        assert latents_out.is_cuda and latents_out.dtype == torch.float32 and latents_out.stride(2) == 1
        assert latents_out.stride(1) == self.d and latents_out.stride(0) % self.d == 0
        return latents_out.stride(0) // self.d

    _NO_SETS = object()          # (an entry without sets arguments; None is an entry called without sets)

    def _sets_args(self, sets, B, warps=True):
        """[sets, warps, n_sets, set_of_row] of a ProcessorSets / WarperSets over B rows, all null for None; warps=False: without them"""
        if sets is not None and len(sets) != B:
            raise ValueError(f"{len(sets)} set indices for {B} rows")
        a = [None, None, 0, None] if sets is None else [sets.sets, getattr(sets, "warps", None), sets.n_sets, sets.set_of_row]
        return a if warps else a[:1] + a[2:]

    def _sample(self, name, logits, ids, ids_len, finished, params, step, rows, extra=(), sets=_NO_SETS, warps=True, need_rows=False):
        """gvc_<name>(logits ... params, rows, *sets arguments, *extra, step, tok, stream) -> the tokens.  sets: the ProcessorSets /
        WarperSets (or None) of the entries that take one, warps=False: of the entry without warpers; need_rows: rows are not optional"""
        B = logits.shape[0]
        if sets is not self._NO_SETS:
            extra = self._sets_args(sets, B, warps) + list(extra)
        tok = torch.empty(B, device=logits.device, dtype=torch.int32)
        arr = _rows_arg(rows, B) if rows is not None or need_rows else None
        check(getattr(lib(), "gvc_" + name)(ptr(_f32(logits)), B, ptr(_i32(ids)), ids.shape[1], ptr(_i32(ids_len)), ptr(_i32(finished)),
                                            C.byref(params), arr, *extra, int(step), ptr(tok), stream()), name)
        return tok

    def _generate(self, name, label, slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out, max_keys, rows,
                  extra=(), sets=_NO_SETS, warps=True, need_rows=False, guided=None, outputs=None):
        """gvc_gpt_<name>(ctx, slots, [uncond_slots,] B, [scale,] ids ... params, rows, *sets arguments, *extra, i0 ... lat_stride,
        [outputs,] stream).  sets, warps, need_rows: as in _sample.
        guided: (uncond_slots or None, scale) of the entries that take them; outputs: (scores_out, logits_out, do_sample) likewise.
        With rows the common params are neutral, whatever the caller passed."""
        self._join_side()
        B = slots.shape[0]
        head = [B]
        if guided is not None:
            uslots, scale = guided
            if uslots is not None and uslots.shape[0] != B:
                raise ValueError(f"{uslots.shape[0]} unconditional slots for {B} items")
            head = [None if uslots is None else ptr(_i32(uslots)), B, float(scale)]
        if sets is not self._NO_SETS:
            extra = self._sets_args(sets, B, warps) + list(extra)
        arr = _rows_arg(rows, B) if rows is not None or need_rows else None
        lat_stride = self._lat_stride(tokens_out, latents_out)
        tail = []
        if outputs is not None:
            out_stride = 0
            for buf in outputs[:2]:
                if buf is not None:
                    if tuple(buf.shape[::2]) != (B, self.V) or (out_stride and buf.shape[1] != out_stride):
                        raise ValueError(f"{name}: an output buffer of shape {tuple(buf.shape)} for {B} rows of {self.V} scores")
                    _f32(buf)
                    out_stride = int(buf.shape[1])
            tail = [ptr(outputs[0]), ptr(outputs[1]), out_stride, int(bool(outputs[2]))]
        if rows is not None:
            params = self._neutral_params()
        check(getattr(lib(), "gvc_gpt_" + name)(self._h, ptr(_i32(slots)), *head, ptr(_i32(ids)), ids.shape[1], ptr(_i32(ids_len)),
                                                ptr(_i32(finished)), C.byref(params), arr, *extra, int(i0), int(n_steps), int(max_keys),
                                                ptr(tokens_out), tokens_out.stride(0), ptr(latents_out), lat_stride, *tail, stream()),
              label)

    def sample(self, logits, ids, ids_len, finished, params, step):
        B = logits.shape[0]
        tok = torch.empty(B, device=logits.device, dtype=torch.int32)
        check(lib().gvc_sample(ptr(_f32(logits)), B, ptr(_i32(ids)), ids.shape[1], ptr(_i32(ids_len)),
                               ptr(_i32(finished)), C.byref(params), step, ptr(tok), stream()), "sample")
        return tok

    def sample_proc(self, logits, ids, ids_len, finished, params, proc, step, rows=None):
        """sample() (rows None) or sample_rows() with the processors `proc` (logits_processors(); include/genvc_hip.h: gvc_sample_proc)"""
        return self._sample("sample_proc", logits, ids, ids_len, finished, params, step, rows, [C.byref(proc)])

    def generate(self, slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out, max_keys=0, proc=None):
        """tokens_out [B, >= i0+n_steps] int32 and latents_out [B, >= i0+n_steps, d] may be column slices of larger
        buffers (row strides are passed on); step i of this call lands in column i0 + i.  max_keys: cached positions of the
        longest stream after the call (0: unknown, the width of `ids` is taken).  proc: the call's processors (logits_processors(),
        include/genvc_hip.h: gvc_gpt_generate_proc) or None."""
        if proc is not None:
            return self._generate("generate_proc", "generate_proc", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out,
                                  latents_out, max_keys, None, [C.byref(proc)])
        # (the plain call stays spelled out: it is the flagship loop's, once per group of steps)
        self._join_side()
        lat_stride = self._lat_stride(tokens_out, latents_out)
        check(lib().gvc_gpt_generate(self._h, ptr(_i32(slots)), slots.shape[0], ptr(_i32(ids)), ids.shape[1], ptr(_i32(ids_len)),
                                     ptr(_i32(finished)), C.byref(params), i0, n_steps, int(max_keys), ptr(tokens_out),
                                     tokens_out.stride(0), ptr(latents_out), lat_stride, stream()), "generate")

    def sample_rows(self, logits, ids, ids_len, finished, rows, step):
        """sample() with per-row settings and RNG keys (include/genvc_hip.h: gvc_sample_rows): row b draws
        rng_uniform(seed_b, rng_step0_b + step, rng_row_b).  rows: see row_sampling()"""
        return self._sample("sample_rows", logits, ids, ids_len, finished, self._neutral_params(), step, rows, need_rows=True)

    def generate_rows(self, slots, ids, ids_len, finished, rows, i0, n_steps, tokens_out, latents_out, max_keys=0, proc=None):
        """generate() with per-row settings and RNG keys (include/genvc_hip.h: gvc_gpt_generate_rows): tokens and latents of step i
        land in column i0 + i as in generate(); row b draws rng_uniform(seed_b, rng_step0_b + i, rng_row_b), so its tokens do not
        depend on which rows share the call.  rows: see row_sampling() (B entries, or a prepared gvc_row_sampling array)"""
        if proc is not None:
            return self._generate("generate_proc", "generate_rows_proc", slots, ids, ids_len, finished, None, i0, n_steps, tokens_out,
                                  latents_out, max_keys, rows, [C.byref(proc)], need_rows=True)
        return self._generate("generate_rows", "generate_rows", slots, ids, ids_len, finished, None, i0, n_steps, tokens_out, latents_out,
                              max_keys, rows, need_rows=True)

    def sample_proc_sets(self, logits, ids, ids_len, finished, params, sets, step, rows=None):
        """sample_proc() with per-row processor sets (logits_processor_sets(); include/genvc_hip.h: gvc_sample_proc_sets): row b uses
        sets.sets[sets.set_of_row[b]], none for -1.  rows: as in sample_proc (then params carries eos / vocab only)"""
        if isinstance(sets, WarperSets):
            return self.sample_warp(logits, ids, ids_len, finished, params, sets, step, rows=rows)
        return self._sample("sample_proc_sets", logits, ids, ids_len, finished, params, step, rows, sets=sets, warps=False)

    def generate_proc_sets(self, slots, ids, ids_len, finished, params, sets, i0, n_steps, tokens_out, latents_out, max_keys=0, rows=None):
        """generate() (rows None: params for every row) or generate_rows() (rows set: params may be None) with per-row processor sets
        (logits_processor_sets(); include/genvc_hip.h: gvc_gpt_generate_proc_sets): row b uses sets.sets[sets.set_of_row[b]], none for
        -1.  The sets travel with the call: the step graphs are generate()'s, and nothing is allocated or captured once warm.
        A WarperSets (logits_sets()) goes to generate_warp()."""
        if isinstance(sets, WarperSets):
            return self.generate_warp(slots, ids, ids_len, finished, params, sets, i0, n_steps, tokens_out, latents_out, max_keys=max_keys,
                                      rows=rows)
        return self._generate("generate_proc_sets", "generate_proc_sets", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out,
                              latents_out, max_keys, rows, sets=sets, warps=False)

    def sample_warp(self, logits, ids, ids_len, finished, params, sets, step, rows=None):
        """sample_proc_sets() with the typical / epsilon / eta warpers of a WarperSets (include/genvc_hip.h: gvc_sample_warp)"""
        return self._sample("sample_warp", logits, ids, ids_len, finished, params, step, rows, sets=sets)

    def generate_warp(self, slots, ids, ids_len, finished, params, sets, i0, n_steps, tokens_out, latents_out, max_keys=0, rows=None):
        """generate_proc_sets() with the warpers of a WarperSets (logits_sets() / WarperSets.one(); include/genvc_hip.h:
        gvc_gpt_generate_warp): row b uses entry sets.set_of_row[b], none for -1.  The warpers travel with the call in one staging
        launch: the step graphs are generate()'s, and nothing is allocated or captured once warm."""
        return self._generate("generate_warp", "generate_warp", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out,
                              max_keys, rows, sets=sets)

    def cfg_guide(self, logits_cond, logits_uncond, scale):
        """HF's classifier-free guidance combine on [B, V] rows (include/genvc_hip.h: gvc_cfg_guide):
        scale * (log_softmax(cond) - log_softmax(uncond)) + log_softmax(uncond)"""
        B, V = logits_cond.shape
        assert logits_uncond.shape == (B, V) and logits_cond.is_cuda and logits_uncond.is_cuda
        out = torch.empty(B, V, device=logits_cond.device, dtype=torch.float32)
        check(lib().gvc_cfg_guide(ptr(_f32(logits_cond)), ptr(_f32(logits_uncond)), B, V, float(scale), ptr(out), stream()), "cfg_guide")
        return out

    def generate_cfg(self, slots, uncond_slots, scale, ids, ids_len, finished, params, sets, i0, n_steps, tokens_out, latents_out,
                     max_keys=0, rows=None):
        """generate_warp() under classifier-free guidance (include/genvc_hip.h: gvc_gpt_generate_cfg): item b decodes in slots[b]
        (conditional prompt) and uncond_slots[b] (unconditional prompt), both prefilled; every step samples item b from
        scale * (lsm(cond) - lsm(uncond)) + lsm(uncond) and feeds the token to both slots.  sets: a WarperSets over the B items, or
        None.  ids / rows / tokens_out / latents_out have B rows: the conditional ones."""
        return self._generate("generate_cfg", "generate_cfg", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out,
                              max_keys, rows, sets=sets, guided=(uncond_slots, scale))

    def generate_scores(self, slots, uncond_slots, scale, ids, ids_len, finished, params, sets, i0, n_steps, tokens_out, latents_out,
                        scores_out=None, logits_out=None, do_sample=True, max_keys=0, rows=None):
        """generate_warp() (uncond_slots None) or generate_cfg() that also stores what every step decoded from (include/genvc_hip.h:
        gvc_gpt_generate_scores): scores_out / logits_out fp32 [B, >= i0 + n_steps, V], dense, either may be None; step i of the call
        lands at [:, i0 + i].  do_sample is HF's flag and decides only what the scores hold: with it the warped row (dropped entries
        -inf), without it the full processed row before any temperature.  sets: a WarperSets over the B rows, or None."""
        return self._generate("generate_scores", "generate_scores", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out,
                              latents_out, max_keys, rows, sets=sets, guided=(uncond_slots, scale),
                              outputs=(scores_out, logits_out, do_sample))

    def sample_bias(self, logits, ids, ids_len, finished, params, bias, step, sets=None, rows=None):
        """sample_warp() with the call's sequence bias / bad words / forced EOS (a _lib.LogitsBias from logits_bias(), or None;
        include/genvc_hip.h: gvc_sample_bias).  sets: a WarperSets / ProcessorSets over the B rows, or None for no processors"""
        return self._sample("sample_bias", logits, ids, ids_len, finished, params, step, rows,
                            [None if bias is None else C.byref(bias)], sets=sets)

    def generate_bias(self, slots, uncond_slots, scale, ids, ids_len, finished, params, sets, bias, i0, n_steps, tokens_out, latents_out,
                      scores_out=None, logits_out=None, do_sample=True, max_keys=0, rows=None):
        """generate_scores() with the call's sequence bias / bad words / forced EOS / renormalised scores (a _lib.LogitsBias from
        logits_bias(); include/genvc_hip.h: gvc_gpt_generate_bias).  The struct travels with the call in one staging launch: the step
        graphs are generate()'s, and nothing is allocated or captured once warm.  bias None is generate_scores()."""
        return self._generate("generate_bias", "generate_bias", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out,
                              max_keys, rows, [None if bias is None else C.byref(bias)], sets=sets,
                              guided=(uncond_slots, scale), outputs=(scores_out, logits_out, do_sample))

    def _ras_args(self, ras, sets, B):
        """[ras table, redraw counters] of a RasTable beside `sets` over B rows"""
        if ras.n != (1 if sets is None else sets.n_sets):
            raise ValueError(f"{ras.n} RAS entries for {1 if sets is None else sets.n_sets} sets")
        if ras.redraws is not None and tuple(ras.redraws.shape) != (B,):
            raise ValueError(f"RAS redraw counters of shape {tuple(ras.redraws.shape)} for {B} rows")
        return [ras.ras, None if ras.redraws is None else ptr(_i32(ras.redraws))]

    def sample_ras(self, logits, ids, ids_len, finished, params, ras, step, sets=None, bias=None, rows=None):
        """sample_bias() with repetition-aware sampling (a RasTable; include/genvc_hip.h: gvc_sample_ras): row b uses entry
        sets.set_of_row[b] of the table (entry 0 without sets, none for -1).  Runs the full kernel whatever top_k is."""
        B = logits.shape[0]
        sa = self._sets_args(sets, B)
        if sets is None:
            sa[2] = 1
        return self._sample("sample_ras", logits, ids, ids_len, finished, params, step, rows,
                            sa + [None if bias is None else C.byref(bias)] + self._ras_args(ras, sets, B))

    def generate_ras(self, slots, uncond_slots, scale, ids, ids_len, finished, params, sets, bias, ras, i0, n_steps, tokens_out,
                     latents_out, scores_out=None, logits_out=None, do_sample=True, max_keys=0, rows=None):
        """generate_bias() with repetition-aware sampling (a RasTable from logits_ras(); include/genvc_hip.h: gvc_gpt_generate_ras).
        The table travels with the call in one staging launch; the step graphs are the sampling ones whatever top_k is
        (warmup(top_k=0) prepares them), and nothing is allocated or captured once warm."""
        B = slots.shape[0]
        sa = self._sets_args(sets, B)
        if sets is None:
            sa[2] = 1
        return self._generate("generate_ras", "generate_ras", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out,
                              max_keys, rows, sa + [None if bias is None else C.byref(bias)] + self._ras_args(ras, sets, B),
                              guided=(uncond_slots, scale), outputs=(scores_out, logits_out, do_sample))

    def _pen_args(self, pen, sets):
        """[penalties table] of a PenaltyTable beside `sets`"""
        if pen.n != (1 if sets is None else sets.n_sets):
            raise ValueError(f"{pen.n} penalty entries for {1 if sets is None else sets.n_sets} sets")
        return [pen.pen]

    def sample_pen(self, logits, ids, ids_len, finished, params, pen, step, sets=None, bias=None, ras=None, rows=None):
        """sample_ras() (ras None: sample_bias()) with the presence / frequency / windowed repetition penalties of a PenaltyTable
        (include/genvc_hip.h: gvc_sample_pen): row b uses entry sets.set_of_row[b] of the table (entry 0 without sets, none for -1).
        The kernel is the one the call runs without the table."""
        B = logits.shape[0]
        sa = self._sets_args(sets, B)
        if sets is None:
            sa[2] = 1
        return self._sample("sample_pen", logits, ids, ids_len, finished, params, step, rows,
                            sa + [None if bias is None else C.byref(bias)] + ([None, None] if ras is None else self._ras_args(ras, sets, B))
                            + self._pen_args(pen, sets))

    def generate_pen(self, slots, uncond_slots, scale, ids, ids_len, finished, params, sets, bias, ras, pen, i0, n_steps, tokens_out,
                     latents_out, scores_out=None, logits_out=None, do_sample=True, max_keys=0, rows=None):
        """generate_ras() (ras None: generate_bias()) with a PenaltyTable from logits_penalties() (include/genvc_hip.h:
        gvc_gpt_generate_pen).  The table travels with the call in one staging launch; the step graphs are those of the call without
        it, and nothing is allocated or captured once warm."""
        B = slots.shape[0]
        sa = self._sets_args(sets, B)
        if sets is None:
            sa[2] = 1
        return self._generate("generate_pen", "generate_pen", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out,
                              max_keys, rows, sa + [None if bias is None else C.byref(bias)]
                              + ([None, None] if ras is None else self._ras_args(ras, sets, B)) + self._pen_args(pen, sets),
                              guided=(uncond_slots, scale), outputs=(scores_out, logits_out, do_sample))

    # ---- green-list watermark: the device-resident tables ----------------------------------------------------------------------
    # One arena of MAX_WATERMARK_TABLES slots of vocab * ceil(vocab / 32) words (135 KB each at vocab 1026), allocated at first use or
    # by GenVCModel.warmup(watermarking_config=...).  A slot is keyed by (hashing_key, ratio, scheme); a WatermarkTable (a call's loop
    # state, a generator, a session) holds its slots while it lives.  Uploads are stream-ordered copies on the caller's stream from a
    # pinned copy of the host table.  A slot is REWRITTEN only when no holder is left and a ninth table needs room, and then only behind
    # torch.cuda.synchronize(): every launch that could still read the old table -- on any stream -- has finished before the copy is
    # enqueued.  A slot that was never written needs no such wait.  Every upload records an event, and every later call that finds the
    # table resident makes its own stream wait for that event, so a call on another stream never reads a table still being copied.
    # The bookkeeping itself is host state of one thread: an engine is driven from one host thread at a time, as its other calls are.
    def _wm_arena(self):
        if getattr(self, "_wm", None) is None:
            words = (self.V + 31) // 32
            self._wm = dict(buf=torch.zeros(MAX_WATERMARK_TABLES, self.V * words, dtype=torch.int32, device="cuda"), words=words,
                            slot={}, holds={}, used=[None] * MAX_WATERMARK_TABLES, tick=0, last={}, pinned={}, uploads=0, ready={})
        return self._wm

    def watermark_entry(self, settings, hold=True):
        """WatermarkSettings -> (gvc_logits_watermark pointing at the settings' device table, the hold's key or None): the table is
        uploaded on the current stream unless a slot already has it.  hold: the slot stays this table until watermark_release(key)
        (WatermarkTable does that).  ValueError: MAX_WATERMARK_TABLES other tables are held."""
        a = self._wm_arena()
        key = (settings.hashing_key, settings.greenlist_ratio, settings.seeding_scheme)
        a["tick"] += 1
        if key not in a["slot"]:
            free = [i for i, k in enumerate(a["used"]) if k is None]
            idle = sorted((a["last"][k], i) for i, k in enumerate(a["used"]) if k is not None and a["holds"].get(k, 0) == 0)
            if free:
                i = free[0]
            elif idle:
                i = idle[0][1]
                torch.cuda.synchronize()          # (nothing that reads the old table is in flight any more, on any stream)
                del a["slot"][a["used"][i]]
            else:
                raise ValueError(f"watermarking_config: {MAX_WATERMARK_TABLES} other watermark tables are in use on this engine "
                                 "(sessions and generators hold theirs while open); close one first")
            host = watermark_table(settings, self.V)
            if key not in a["pinned"]:
                a["pinned"] = {key: host.view(torch.int32).reshape(-1).pin_memory()}          # (one pinned staging copy at a time)
            src = a["pinned"][key]
            a["buf"][i, :src.numel()].copy_(src, non_blocking=True)
            a["ready"][key] = torch.cuda.Event()
            a["ready"][key].record()          # (a call on another stream waits for this copy: below)
            a["used"][i] = key
            a["slot"][key] = i
            a["uploads"] += 1
        i = a["slot"][key]
        torch.cuda.current_stream().wait_event(a["ready"][key])          # (the upload may have been enqueued on another stream)
        a["last"][key] = a["tick"]
        if hold:
            a["holds"][key] = a["holds"].get(key, 0) + 1
        m = _lib.LogitsWatermark(a["buf"][i].data_ptr(), float(settings.bias), WATERMARK_SCHEMES[settings.seeding_scheme], a["words"], 0)
        return m, (key if hold else None)

    def watermark_release(self, key):
        a = getattr(self, "_wm", None)
        if a is not None and a["holds"].get(key, 0) > 0:
            a["holds"][key] -= 1

    def watermark_uploads(self):
        """how many tables this engine has uploaded (a warm marked call uploads none)"""
        a = getattr(self, "_wm", None)
        return 0 if a is None else a["uploads"]

    def _wm_args(self, wm, sets):
        """[watermark entries] of a WatermarkTable beside `sets`"""
        if wm.n != (1 if sets is None else sets.n_sets):
            raise ValueError(f"{wm.n} watermark entries for {1 if sets is None else sets.n_sets} sets")
        return [wm.wm]

    def sample_wm(self, logits, ids, ids_len, finished, params, wm, step, sets=None, bias=None, ras=None, pen=None, rows=None):
        """sample_pen() (pen None: sample_ras() ...) with the green-list watermark of a WatermarkTable (include/genvc_hip.h:
        gvc_sample_wm): row b uses entry sets.set_of_row[b] of the table (entry 0 without sets, none for -1).  The kernel is the one
        the call runs without the table."""
        B = logits.shape[0]
        sa = self._sets_args(sets, B)
        if sets is None:
            sa[2] = 1
        return self._sample("sample_wm", logits, ids, ids_len, finished, params, step, rows,
                            sa + [None if bias is None else C.byref(bias)] + ([None, None] if ras is None else self._ras_args(ras, sets, B))
                            + ([None] if pen is None else self._pen_args(pen, sets)) + self._wm_args(wm, sets))

    def generate_wm(self, slots, uncond_slots, scale, ids, ids_len, finished, params, sets, bias, ras, pen, wm, i0, n_steps, tokens_out,
                    latents_out, scores_out=None, logits_out=None, do_sample=True, max_keys=0, rows=None):
        """generate_pen() (pen None: generate_ras() ...) with a WatermarkTable (include/genvc_hip.h: gvc_gpt_generate_wm).  The entries
        travel with the call in one staging launch; the step graphs are those of the call without them, and nothing is allocated or
        captured once the tables are resident."""
        B = slots.shape[0]
        sa = self._sets_args(sets, B)
        if sets is None:
            sa[2] = 1
        return self._generate("generate_wm", "generate_wm", slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out,
                              max_keys, rows, sa + [None if bias is None else C.byref(bias)]
                              + ([None, None] if ras is None else self._ras_args(ras, sets, B))
                              + ([None] if pen is None else self._pen_args(pen, sets)) + self._wm_args(wm, sets),
                              guided=(uncond_slots, scale), outputs=(scores_out, logits_out, do_sample))

    def generate_call(self, slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out, max_keys=0, rows=None, proc=None,
                      sets=None, bias=None, uncond_slots=None, scale=1.0, scores_out=None, logits_out=None, do_sample=True, ras=None,
                      pen=None, wm=None):
        """The generation call for whatever options a loop has, through the narrowest entry that carries them: generate_bias (bias),
        generate_scores (score / logit buffers), generate_cfg (uncond_slots), generate_proc_sets / generate_warp (sets), generate_rows
        (rows), else generate.  proc: the call-wide processors; sets (a ProcessorSets / WarperSets) supersedes it, and the entries
        without a `proc` argument take it as one call-wide entry.  A loop makes this one call instead of choosing.  It goes through
        the public methods, so a patched or overridden entry still sees its calls, and an engine stand-in that has no generate_call
        of its own (layers.gpt._generate_call) needs only the entries its options reach."""
        wide = (bias is not None or scores_out is not None or logits_out is not None or uncond_slots is not None or ras is not None
                or pen is not None or wm is not None)
        if wide and sets is None and proc is not None:
            sets = WarperSets.one(proc, None, slots.shape[0])
        pk = {} if proc is None or sets is not None else {"proc": proc}
        if ras is None:
            ras = getattr(sets, "ras", None)          # (per-row entries ride with the sets: logits_sets)
        if pen is None:
            pen = getattr(sets, "pen", None)
        if wm is None:
            wm = getattr(sets, "wm", None)
        if wm is not None:           # (a WatermarkTable: the green-list watermark, the widest entry)
            return self.generate_wm(slots, uncond_slots, scale, ids, ids_len, finished, params, sets, bias, ras, pen, wm, i0, n_steps,
                                    tokens_out, latents_out, scores_out=scores_out, logits_out=logits_out, do_sample=do_sample,
                                    max_keys=max_keys, rows=rows)
        if pen is not None:          # (a PenaltyTable: presence / frequency / windowed penalties, the widest entry)
            return self.generate_pen(slots, uncond_slots, scale, ids, ids_len, finished, params, sets, bias, ras, pen, i0, n_steps,
                                     tokens_out, latents_out, scores_out=scores_out, logits_out=logits_out, do_sample=do_sample,
                                     max_keys=max_keys, rows=rows)
        if ras is not None:          # (a RasTable: repetition-aware sampling)
            return self.generate_ras(slots, uncond_slots, scale, ids, ids_len, finished, params, sets, bias, ras, i0, n_steps, tokens_out,
                                     latents_out, scores_out=scores_out, logits_out=logits_out, do_sample=do_sample, max_keys=max_keys,
                                     rows=rows)
        if bias is not None:
            return self.generate_bias(slots, uncond_slots, scale, ids, ids_len, finished, params, sets, bias, i0, n_steps, tokens_out,
                                      latents_out, scores_out=scores_out, logits_out=logits_out, do_sample=do_sample, max_keys=max_keys,
                                      rows=rows)
        if scores_out is not None or logits_out is not None:
            return self.generate_scores(slots, uncond_slots, scale, ids, ids_len, finished, params, sets, i0, n_steps, tokens_out,
                                        latents_out, scores_out=scores_out, logits_out=logits_out, do_sample=do_sample, max_keys=max_keys,
                                        rows=rows)
        if uncond_slots is not None:
            return self.generate_cfg(slots, uncond_slots, scale, ids, ids_len, finished, params, sets, i0, n_steps, tokens_out, latents_out,
                                     max_keys=max_keys, rows=rows)
        if sets is not None:
            return self.generate_proc_sets(slots, ids, ids_len, finished, params, sets, i0, n_steps, tokens_out, latents_out,
                                           max_keys=max_keys, rows=rows)
        if rows is not None:
            return self.generate_rows(slots, ids, ids_len, finished, rows, i0, n_steps, tokens_out, latents_out, max_keys=max_keys, **pk)
        return self.generate(slots, ids, ids_len, finished, params, i0, n_steps, tokens_out, latents_out, max_keys=max_keys, **pk)

    def transition_scores(self, scores, tokens, normalize=False):
        """HF's compute_transition_scores without beams on the device (include/genvc_hip.h: gvc_transition_scores): scores fp32
        [R, n, V] (its rows dense, the stride between rows free: a column slice of a generate_scores buffer goes in as it is), tokens
        int32 [R, n] -> fp32 [R, n]: scores[r, t, tokens[r, t]], behind a log_softmax over the vocabulary when normalize"""
        assert scores.is_cuda and scores.dtype == torch.float32 and scores.ndim == 3
        R, n, V = scores.shape
        if tuple(tokens.shape) != (R, n):
            raise ValueError(f"transition_scores: tokens {tuple(tokens.shape)} do not go with scores {tuple(scores.shape)}")
        if n == 0 or R == 0:
            return torch.empty(R, n, device=scores.device, dtype=torch.float32)
        if scores.stride(2) != 1 or scores.stride(1) != V or (R > 1 and scores.stride(0) < n * V):
            scores = scores.contiguous()
        out = torch.empty(R, n, device=scores.device, dtype=torch.float32)
        check(lib().gvc_transition_scores(ptr(scores), int(scores.stride(0)) if R > 1 else n * V, ptr(_i32(tokens.contiguous())), R, n, V,
                                          int(bool(normalize)), ptr(out), stream()), "transition_scores")
        return out

    def warmup_cfg(self, B, max_keys=0, top_k=1):
        """warmup() for generate_cfg over B items (include/genvc_hip.h: gvc_gpt_warmup_cfg)"""
        check(lib().gvc_gpt_warmup_cfg(self._h, int(B), int(max_keys), int(top_k)), "warmup_cfg")

    def verify(self, slots, toks, logits=None, latent=None):
        """T = toks.shape[1] new rows per slot in one pass (include/genvc_hip.h: gvc_gpt_verify): toks int32 [B, T] ->
        (logits [B, T, V], latent [B, T, d]) of every row; the slots' lengths and mel positions grow by T"""
        self._join_side()
        B, T = toks.shape
        if slots.shape[0] != B:
            raise ValueError(f"{slots.shape[0]} slots for {B} rows of tokens")
        if logits is None:
            logits = torch.empty(B, T, self.V, device=toks.device, dtype=torch.float32)
            latent = torch.empty(B, T, self.d, device=toks.device, dtype=torch.float32)
        check(lib().gvc_gpt_verify(self._h, ptr(_i32(slots)), B, ptr(_i32(toks)), T, ptr(_f32(logits)), ptr(_f32(latent)), stream()),
              "verify")
        return logits, latent

    def truncate(self, slots, drop):
        """roll the slots back by drop[b] positions (device int32 [B]; include/genvc_hip.h: gvc_gpt_truncate); no synchronisation"""
        if drop.shape[0] != slots.shape[0]:
            raise ValueError(f"{drop.shape[0]} drop counts for {slots.shape[0]} slots")
        check(lib().gvc_gpt_truncate(self._h, ptr(_i32(slots)), slots.shape[0], ptr(_i32(drop)), stream()), "truncate")

    def generate_assisted(self, assistant, slots, assistant_slots, state, params, n_rounds, max_keys, assistant_max_keys, proc=None,
                          k=None, sampling=False):
        """n_rounds rounds of assisted greedy decoding of `state` (an AssistedState) with this engine as the target and `assistant`
        (another GptEngine) drafting k (default state.k; never more) tokens per round (include/genvc_hip.h:
        gvc_gpt_generate_assisted).  The first call of a state also runs its opening step.  max_keys / assistant_max_keys: cached positions the longest stream reaches inside the call.
        sampling=True: speculative sampling with every sampling field of `params` (gvc_gpt_generate_assisted_sample; top_k != 1); the
        state gets its sampling workspaces on the first such call"""
        self._join_side()
        assistant._join_side()
        if slots.shape[0] != state.B or assistant_slots.shape[0] != state.B:
            raise ValueError(f"{slots.shape[0]} / {assistant_slots.shape[0]} slots for {state.B} streams")
        k = state.k if k is None else int(k)
        if not 1 <= k <= state.k:
            raise ValueError(f"{k} drafts per round outside [1, {state.k}]")
        if sampling:
            check(lib().gvc_gpt_generate_assisted_sample(self._h, assistant._h, ptr(_i32(slots)), ptr(_i32(assistant_slots)),
                                                         C.byref(state.c), C.byref(state.sampling()), C.byref(params),
                                                         None if proc is None else C.byref(proc), int(not state.opened), int(n_rounds), k,
                                                         int(max_keys), int(assistant_max_keys), stream()),
                  "generate_assisted_sample")
        else:
            check(lib().gvc_gpt_generate_assisted(self._h, assistant._h, ptr(_i32(slots)), ptr(_i32(assistant_slots)), C.byref(state.c),
                                                  C.byref(params), None if proc is None else C.byref(proc), int(not state.opened),
                                                  int(n_rounds), k, int(max_keys), int(assistant_max_keys), stream()),
                  "generate_assisted")
        state.opened = True
        state.rounds_done += int(n_rounds)

    def generate_lookup(self, slots, state, params, n_rounds, max_keys, max_ngram, proc=None, k=None, sampling=False):
        """n_rounds rounds of prompt-lookup assisted decoding of `state` (an AssistedState) on this engine alone (include/genvc_hip.h:
        gvc_gpt_generate_lookup): every round drafts up to k (default state.k; never more) tokens per row from the row's own generated
        ids -- the longest suffix of up to max_ngram ids that occurs earlier in ids[state.n0 ..] -- and otherwise runs as a round of
        generate_assisted.  The first call of a state also runs its opening step.  sampling=True: speculative sampling with one-hot
        draft rows and every sampling field of `params` (top_k != 1)"""
        self._join_side()
        if slots.shape[0] != state.B:
            raise ValueError(f"{slots.shape[0]} slots for {state.B} streams")
        k = state.k if k is None else int(k)
        if not 1 <= k <= state.k:
            raise ValueError(f"{k} drafts per round outside [1, {state.k}]")
        check(lib().gvc_gpt_generate_lookup(self._h, ptr(_i32(slots)), C.byref(state.c), C.byref(state.sampling()) if sampling else None,
                                            C.byref(params), None if proc is None else C.byref(proc), int(not state.opened),
                                            int(n_rounds), k, int(max_ngram), state.n0, ptr(state.draft_len), int(max_keys), stream()),
              "generate_lookup")
        state.opened = True
        state.rounds_done += int(n_rounds)

    def beam_generate(self, slots, beam, n_steps, max_keys=0):
        """n_steps steps of `beam` (a BeamSearch) on the device, continuing at beam.steps (include/genvc_hip.h: gvc_gpt_beam_generate):
        item b was prefilled into slots[b*K]; slots [B*K] int32 is rewritten to the beams' slots"""
        self._join_side()
        if beam.proc is not None:
            check(lib().gvc_gpt_beam_generate_proc(self._h, ptr(_i32(slots)), C.byref(beam.c), C.byref(beam.proc), int(beam.steps),
                                                   int(n_steps), int(max_keys), stream()), "beam_generate_proc")
        else:
            check(lib().gvc_gpt_beam_generate(self._h, ptr(_i32(slots)), C.byref(beam.c), int(beam.steps), int(n_steps), int(max_keys),
                                              stream()), "beam_generate")
        beam.steps += int(n_steps)

    def prefill_hidden(self, slots, prefix_emb, hidden_out):
        """prefill (logits and latent parked per slot) that also writes hidden_out [B, P+1, d] = ln_f of every row
        (include/genvc_hip.h: gvc_gpt_prefill_hidden)"""
        self._join_side()
        B, P, _ = prefix_emb.shape
        assert hidden_out.shape == (B, P + 1, self.d)
        check(lib().gvc_gpt_prefill_hidden(self._h, ptr(_i32(slots)), B, ptr(_f32(prefix_emb)), P, self.dims["start_audio_token"],
                                           ptr(_f32(hidden_out)), stream()), "prefill_hidden")

    def contrastive_generate(self, slots, cs, n_steps, max_keys=0):
        """n_steps steps of `cs` (a ContrastiveSearch) on the device, continuing at cs.steps (include/genvc_hip.h:
        gvc_gpt_contrastive_generate): item b was prefilled into slots[b*K] with prefill_hidden(..., cs.hidden0)"""
        self._join_side()
        if cs.proc is not None:
            check(lib().gvc_gpt_contrastive_generate_proc(self._h, ptr(_i32(slots)), C.byref(cs.c), C.byref(cs.proc), int(cs.steps),
                                                          int(n_steps), int(max_keys), stream()), "contrastive_generate_proc")
        else:
            check(lib().gvc_gpt_contrastive_generate(self._h, ptr(_i32(slots)), C.byref(cs.c), int(cs.steps), int(n_steps), int(max_keys),
                                                     stream()), "contrastive_generate")
        cs.steps += int(n_steps)

    def warmup_contrastive(self, B, K, max_keys=0):
        """warmup() for contrastive_generate over B items of K candidates (include/genvc_hip.h: gvc_gpt_warmup_contrastive)"""
        check(lib().gvc_gpt_warmup_contrastive(self._h, int(B), int(K), int(max_keys)), "warmup_contrastive")

    def group_beam_generate(self, slots, beam, n_steps, max_keys=0):
        """beam_generate for a GroupBeamSearch (include/genvc_hip.h: gvc_gpt_group_beam_generate): with G > 1 the first call fans the
        prefilled slot of every item out to its other K-1 slots before the first step"""
        self._join_side()
        check(lib().gvc_gpt_group_beam_generate(self._h, ptr(_i32(slots)), C.byref(beam.c), C.byref(beam.g),
                                                C.byref(beam.proc) if beam.proc is not None else None, int(beam.steps), int(n_steps),
                                                int(max_keys), stream()), "group_beam_generate")
        beam.steps += int(n_steps)

    def warmup_group_beam(self, B, K, G, max_keys=0):
        """warmup() for group_beam_generate over B items of K beams in G groups (include/genvc_hip.h: gvc_gpt_warmup_group_beam)"""
        check(lib().gvc_gpt_warmup_group_beam(self._h, int(B), int(K), int(G), int(max_keys)), "warmup_group_beam")

    def warmup_beam(self, B, K, max_keys=0):
        """warmup() for beam_generate over B items of K beams (include/genvc_hip.h: gvc_gpt_warmup_beam)"""
        check(lib().gvc_gpt_warmup_beam(self._h, int(B), int(K), int(max_keys)), "warmup_beam")

    def decode_variant(self):
        """which decode step the last generate() call replayed (include/genvc_hip.h: gvc_gpt_decode_variant)"""
        return int(lib().gvc_gpt_decode_variant(self._h))

    def health(self):
        """after a synchronisation: raises if the work just finished hit a hand-off timeout (the context then continues on the
        launch-per-phase paths) or a full KV cache (include/genvc_hip.h: gvc_gpt_health)"""
        check(lib().gvc_gpt_health(self._h), "health")

    def warmup(self, B=1, max_keys=0, top_k=1):
        """everything the first generate / decode_step / cached prefill of this shape would do on first use (buffers, weight pack,
        topology probe, step-graph capture); afterwards such calls neither allocate nor synchronise (include/genvc_hip.h: gvc_gpt_warmup)"""
        check(lib().gvc_gpt_warmup(self._h, int(B), int(max_keys), int(top_k)), "warmup")

    def lazy_inits(self):
        """allocations / device syncs / graph captures done inside data-path calls so far (include/genvc_hip.h: gvc_gpt_lazy_inits)"""
        return int(lib().gvc_gpt_lazy_inits(self._h))

    def warmup_range(self, B, min_keys, max_keys, top_k=1):
        """warm-up of every context class a generation passes through while its longest stream grows from min_keys to max_keys cached
        positions (include/genvc_hip.h: gvc_gpt_warmup_range -- the library enumerates its own classes)"""
        check(lib().gvc_gpt_warmup_range(self._h, B, min_keys, max_keys, top_k), "warmup_range")

    def rearm(self):
        """back to the one-launch steps after a time-out fallback, when the GPU is the caller's own again (include/genvc_hip.h: gvc_gpt_rearm)"""
        check(lib().gvc_gpt_rearm(self._h), "rearm")

    def one_stream_steps(self):
        """one-stream one-launch decode steps that ran so far, early exits of deferred decodes not counted; synchronises the device
        (include/genvc_hip.h: gvc_gpt_one_stream_steps)"""
        return int(lib().gvc_gpt_one_stream_steps(self._h))

    def rows_step_launches(self):
        """one-launch rows steps issued so far (include/genvc_hip.h: gvc_gpt_rows_step_launches)"""
        return int(lib().gvc_gpt_rows_step_launches(self._h))

    def bf16_gemm_launches(self):
        """bf16 matrix-core strip GEMMs issued so far: the multi-row passes of a "bf16_mfma" context (gvc_gpt_bf16_gemm_launches)"""
        return int(lib().gvc_gpt_bf16_gemm_launches(self._h))

    def time_kernel(self, which, slots, tok, n_steps):
        """(mean us per launch, launches) of one kernel class of the decode step, launched back to back"""
        avg, n = C.c_float(), C.c_int32()
        check(lib().gvc_gpt_time_kernel(self._h, which, ptr(_i32(slots)), slots.shape[0], ptr(_i32(tok)), n_steps,
                                        C.byref(avg), C.byref(n), stream()), "time_kernel")
        return avg.value, n.value


class PerceiverEngine:
    """PerceiverResampler.forward (reference layers/perceiver_encoder.py:265-276)."""

    def __init__(self, dim, depth=2, dim_context=None, num_latents=32, dim_head=64, heads=8, ff_mult=4,
                 max_batch=8, max_frames=2816):
        dim_context = dim if dim_context is None else dim_context
        self.dim, self.num_latents, self.dim_context = dim, num_latents, dim_context
        cd = _lib.PerceiverDims(dim, depth, dim_context, num_latents, dim_head, heads, ff_mult, max_batch, max_frames)
        self._h = C.c_void_p()
        check(lib().gvc_perceiver_create(C.byref(cd), C.byref(self._h)), "gvc_perceiver_create")

    def close(self):
        if self._h:
            lib().gvc_perceiver_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, weights, prefix=""):
        for name, t in weights.items():
            if not name.startswith(prefix) or not torch.is_tensor(t):
                continue
            t = _f32(t.detach().to(torch.float32).contiguous())
            check(lib().gvc_perceiver_bind_weight(self._h, name[len(prefix):].encode(), ptr(t), t.numel(), stream()),
                  f"bind {name}")
        torch.cuda.current_stream().synchronize()
        missing = lib().gvc_perceiver_missing_weights(self._h)
        if missing:
            raise _lib.GenvcHipError(f"{missing} Perceiver weight tensors missing after bind")

    def forward_masked(self, x, key_mask):
        """x [B, F, dim_context], key_mask uint8 / bool [B, num_latents + F] over the keys [latents | frames] (nonzero = attend)
        (include/genvc_hip.h: gvc_perceiver_forward_masked)"""
        B, F, _ = x.shape
        if tuple(key_mask.shape) != (B, self.num_latents + F):
            raise ValueError(f"perceiver: mask {tuple(key_mask.shape)} for {B} x ({self.num_latents} latents + {F} frames)")
        key_mask = key_mask.to(device=x.device, dtype=torch.uint8).contiguous()
        out = torch.empty(B, self.num_latents, self.dim, device=x.device, dtype=torch.float32)
        check(lib().gvc_perceiver_forward_masked(self._h, ptr(_f32(x)), B, F, ptr(key_mask), ptr(out), stream()), "perceiver_forward_masked")
        return out

    def forward(self, x):
        """x [B,F,dim_context] -> [B,num_latents,dim]"""
        B, F, _ = x.shape
        out = torch.empty(B, self.num_latents, self.dim, device=x.device, dtype=torch.float32)
        check(lib().gvc_perceiver_forward(self._h, ptr(_f32(x)), B, F, ptr(out), stream()), "perceiver_forward")
        return out


class MelEngine:
    """TorchMelSpectrogram.forward (reference utils.py:150-162)."""

    def __init__(self, mel_norms, n_fft=2048, hop=256, win=1024, sample_rate=24000, f_min=0.0, f_max=8000.0, n_mels=80):
        import numpy as np
        norms = np.ascontiguousarray(np.asarray(mel_norms, dtype=np.float32))
        assert norms.shape == (n_mels,)
        self.hop, self.n_mels = hop, n_mels
        self._h = C.c_void_p()
        check(lib().gvc_mel_create(n_fft, hop, win, sample_rate, f_min, f_max, n_mels,
                                   norms.ctypes.data_as(_lib.c_f32p), C.byref(self._h)), "gvc_mel_create")

    def close(self):
        if self._h:
            lib().gvc_mel_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, wav, frames_major=False):
        """wav [B,T] -> [B,n_mels,1+T//hop]  (and [B,1+T//hop,n_mels] when frames_major)"""
        B, T = wav.shape
        nf = 1 + T // self.hop
        out = torch.empty(B, self.n_mels, nf, device=wav.device, dtype=torch.float32)
        fm = torch.empty(B, nf, self.n_mels, device=wav.device, dtype=torch.float32) if frames_major else None
        check(lib().gvc_mel_forward(self._h, ptr(_f32(wav)), B, T, ptr(out), ptr(fm), stream()), "mel_forward")
        return (out, fm) if frames_major else out


class GriffinLimEngine:
    """TorchMelSpectrogram.invert (reference utils.py:164-172) in its parts: the inverse mel scale (torchaudio's InverseMelScale: the
    minimum-norm least-squares inverse of the filterbank, relu'd) and librosa.griffinlim (csrc/griffinlim.hip).  `max_batch` and
    `max_frames` bound griffinlim(); a filterbank without an inverse raises ValueError naming the filter."""

    def __init__(self, mel_norms=None, n_fft=1024, hop=256, win=1024, sample_rate=22050, f_min=0.0, f_max=8000.0, n_mels=80,
                 max_batch=1, max_frames=1024):
        import numpy as np
        norms = None
        if mel_norms is not None:
            norms = np.ascontiguousarray(np.asarray(mel_norms, dtype=np.float32))
            assert norms.shape == (n_mels,)
        o = _lib.GlOptions()
        o.n_fft, o.hop, o.win, o.sample_rate, o.n_mels = n_fft, hop, win, sample_rate, n_mels
        o.max_batch, o.max_frames = max_batch, max_frames
        o.f_min, o.f_max = float(f_min), float(f_max)
        self.n_fft, self.hop, self.win, self.n_mels, self.n_freq = n_fft, hop, win, n_mels, n_fft // 2 + 1
        self.max_batch, self.max_frames = max_batch, max_frames
        self._h = C.c_void_p()
        rc = lib().gvc_gl_create(C.byref(o), None if norms is None else norms.ctypes.data_as(_lib.c_f32p), C.byref(self._h))
        if rc == -1:        # GVC_ERR_ARG: an unsupported configuration, or a filterbank without an inverse (the message names the filter)
            raise ValueError(lib().gvc_last_error().decode(errors="replace"))
        check(rc, "gvc_gl_create")

    def close(self):
        if self._h:
            lib().gvc_gl_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def inverse_matrix(self):
        """W float32 [n_freq, n_mels] = fb (fb^T fb)^-1 (a host tensor)"""
        w = torch.empty(self.n_freq, self.n_mels, dtype=torch.float32)
        check(lib().gvc_gl_inverse_matrix(self._h, C.cast(w.data_ptr(), _lib.c_f32p)), "gl_inverse_matrix")
        return w

    def inverse_mel(self, mel):
        """mel [B,n_mels,F] (normalised log power mel) -> S [B,n_freq,F] = relu(W exp(mel * norms))"""
        B, _, F = mel.shape
        out = torch.empty(B, self.n_freq, F, device=mel.device, dtype=torch.float32)
        check(lib().gvc_gl_inverse_mel(self._h, ptr(_f32(mel)), B, F, ptr(out), stream()), "gl_inverse_mel")
        return out

    def init_angles(self, seed, B, F):
        """complex64 [B,n_freq,F] unit phasors exp(2 pi i u), u from the sampler's counter-based generator keyed by (seed, item, bin, frame)"""
        out = torch.empty(B, self.n_freq, F, device="cuda", dtype=torch.complex64)
        check(lib().gvc_gl_init_angles(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, B, F, ptr(out), stream()), "gl_init_angles")
        return out

    def griffinlim(self, S, init_angles=None, seed=0, n_iter=64, momentum=0.99):
        """S [B,n_freq,F] -> wav [B, hop (F - 1)] after n_iter iterations from init_angles (or the seeded start)"""
        B, _, F = S.shape
        if init_angles is None:
            init_angles = self.init_angles(seed, B, F)
        S, init_angles = _f32(S), init_angles.contiguous()
        wav = torch.empty(B, self.hop * (F - 1), device=S.device, dtype=torch.float32)
        check(lib().gvc_gl_run(self._h, ptr(S), ptr(init_angles), B, F, int(n_iter), float(momentum), ptr(wav), stream()), "gl_run")
        return wav

    def launches(self):
        """kernel launches enqueued so far (measurement)"""
        return int(lib().gvc_gl_launches(self._h))


class DvaeEngine:
    """DiscreteVAE.get_codebook_indices (reference layers/dvae.py:324-331); with_decoder=True: also decode (:333-352) and the
    eval-mode forward (:363-381)."""

    def __init__(self, cfg, max_batch=8, max_frames=1504, with_decoder=False):
        self.cfg = dict(cfg)
        self.with_decoder = bool(with_decoder)
        cd = _lib.DvaeDims(cfg["num_channels"], cfg["hidden_dim"], cfg["num_layers"], cfg["num_resnet_blocks"],
                           cfg["kernel_size"], cfg["codebook_dim"], cfg["num_tokens"], max_batch, max_frames)
        self._h = C.c_void_p()
        if self.with_decoder:
            check(lib().gvc_dvae_create_ex(C.byref(cd), _lib.DVAE_DECODER, C.byref(self._h)), "gvc_dvae_create_ex")
        else:
            check(lib().gvc_dvae_create(C.byref(cd), C.byref(self._h)), "gvc_dvae_create")

    def close(self):
        if self._h:
            lib().gvc_dvae_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, weights, prefix=""):
        for name, t in weights.items():
            if not name.startswith(prefix) or not torch.is_tensor(t) or not t.is_floating_point():
                continue
            t = _f32(t.detach().to(torch.float32).contiguous())
            check(lib().gvc_dvae_bind_weight(self._h, name[len(prefix):].encode(), ptr(t), t.numel(), stream()),
                  f"bind {name}")
        torch.cuda.current_stream().synchronize()
        missing = lib().gvc_dvae_missing_weights(self._h)
        if missing:
            raise _lib.GenvcHipError(f"{missing} DVAE weight tensors missing after bind")

    def out_frames(self, T):
        k = self.cfg["kernel_size"]
        for _ in range(self.cfg["num_layers"]):
            T = (T + 2 * ((k - 1) // 2) - k) // 2 + 1
        return T

    def encode(self, feat, return_enc=False, frames_major=False):
        """feat [B,C,T] (or [B,T,C] with frames_major) -> int32 codes [B,Tc] (and the encoder output [B,Tc,codebook_dim])"""
        if frames_major:
            B, T, _ = feat.shape
        else:
            B, _, T = feat.shape
        Tc = self.out_frames(T)
        codes = torch.empty(B, Tc, device=feat.device, dtype=torch.int32)
        enc = torch.empty(B, Tc, self.cfg["codebook_dim"], device=feat.device, dtype=torch.float32) if return_enc else None
        fn = lib().gvc_dvae_encode_frames if frames_major else lib().gvc_dvae_encode
        check(fn(self._h, ptr(_f32(feat)), B, T, ptr(codes), ptr(enc), stream()), "dvae_encode")
        return (codes, enc) if return_enc else codes

    def decode(self, codes, return_pre=True):
        """codes int32 [B,n] -> out [B,channels,n 2^L] (and the last layer's input [B,hidden,n 2^L]).  Synchronises to learn
        whether a code was out of range (ValueError)."""
        B, n = codes.shape
        T = n << self.cfg["num_layers"]
        codes = codes.to(torch.int32).contiguous()
        out = torch.empty(B, self.cfg["num_channels"], T, device=codes.device, dtype=torch.float32)
        pre = torch.empty(B, self.cfg["hidden_dim"], T, device=codes.device, dtype=torch.float32) if return_pre else None
        check(lib().gvc_dvae_decode(self._h, ptr(codes), B, n, ptr(out), ptr(pre), stream()), "dvae_decode")
        if lib().gvc_dvae_code_error(self._h, stream()) != 0:
            raise ValueError(lib().gvc_last_error().decode(errors="replace"))
        return (out, pre) if return_pre else out

    def reconstruct(self, feat):
        """feat [B,channels,T] -> (losses float32 [2] = (recon, commitment), out [B,channels,T], codes int32 [B,T / 2^L])"""
        B, _, T = feat.shape
        feat = _f32(feat)
        out = torch.empty_like(feat)
        codes = torch.empty(B, T >> self.cfg["num_layers"], device=feat.device, dtype=torch.int32)
        losses = torch.empty(2, device=feat.device, dtype=torch.float32)
        check(lib().gvc_dvae_reconstruct(self._h, ptr(feat), B, T, ptr(out), ptr(codes), ptr(losses), stream()), "dvae_reconstruct")
        return losses, out, codes


def vq_argmin(x, embed):
    """x [N,dim], embed [dim,n_embed] -> int32 [N] (Quantize.forward, reference layers/dvae.py:87-90)."""
    N, dim = x.shape
    idx = torch.empty(N, device=x.device, dtype=torch.int32)
    work = torch.empty(N * embed.shape[1], device=x.device, dtype=torch.float32)
    check(lib().gvc_vq_argmin(ptr(_f32(x)), ptr(_f32(embed)), N, dim, embed.shape[1], ptr(idx), ptr(work), stream()),
          "vq_argmin")
    return idx


class HifiganEngine:
    """HiFiGAN.forward (reference layers/hifigan.py:218-233) and the latent entry point with the x4 interpolation."""

    def __init__(self, cfg, max_batch=2, max_frames=2560):
        self.cfg = dict(cfg)
        # the reference's rule (layers/hifigan.py:181): "1" is ResBlock1, anything else ResBlock2
        self.resblock_type = 1 if str(cfg.get("resblock_type", "2")) == "1" else 2
        d = _lib.HifiganDimsEx() if self.resblock_type == 1 else _lib.HifiganDims()
        d.in_dim, d.up_init_ch = cfg["input_feat_dim"], cfg["upsample_initial_channel"]
        d.n_ups, d.n_kernels = len(cfg["upsample_rates"]), len(cfg["resblock_kernel_sizes"])
        for i, (r, k) in enumerate(zip(cfg["upsample_rates"], cfg["upsample_kernel_sizes"])):
            d.up_rates[i], d.up_kernels[i] = r, k
        for j, (k, dl) in enumerate(zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"])):
            d.res_kernels[j] = k
            if self.resblock_type == 1:
                if len(dl) != 3:
                    raise ValueError(f"HiFi-GAN ResBlock1 takes 3 dilations per kernel, got {list(dl)}")
                d.res_dilations[j][0], d.res_dilations[j][1], d.res_dilations[j][2] = dl
            else:
                d.res_dilations[j][0], d.res_dilations[j][1] = dl
        if self.resblock_type == 1:
            d.resblock_type = 1
        d.max_batch, d.max_frames = max_batch, max_frames
        self.max_frames = max_frames
        self.total_up = 1
        for r in cfg["upsample_rates"]:
            self.total_up *= r
        self.in_dim = cfg["input_feat_dim"]
        self._h = C.c_void_p()
        if self.resblock_type == 1:
            check(lib().gvc_hifigan_create_ex(C.byref(d), C.byref(self._h)), "gvc_hifigan_create_ex")
        else:
            check(lib().gvc_hifigan_create(C.byref(d), C.byref(self._h)), "gvc_hifigan_create")

    @property
    def lds_stages(self):
        """upsampling stages whose ResBlocks run on the one-round-trip conv kernel (the rest: one tiled-GEMM launch per conv)"""
        return lib().gvc_hifigan_lds_stages(self._h)

    @property
    def graph_nodes(self):
        """nodes of the most recently captured whole-call graph (its launches: input staging .. conv_post)"""
        return lib().gvc_hifigan_graph_nodes(self._h)

    def close(self):
        if self._h:
            lib().gvc_hifigan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, weights, prefix=""):
        """weights: reference state dict; weight-norm pairs (weight_g, weight_v) are folded here (loader plumbing)."""
        sd = {k[len(prefix):]: v for k, v in weights.items() if k.startswith(prefix) and torch.is_tensor(v)}
        folded = {}
        for k, v in sd.items():
            if k.endswith(".weight_v"):
                g = sd[k[:-2] + "_g"]
                norm = v.float().pow(2).sum(dim=tuple(range(1, v.dim())), keepdim=True).sqrt()
                folded[k[:-9] + ".weight"] = (g.float() * v.float() / norm)
            elif k.endswith(".weight_g"):
                continue
            else:
                folded[k] = v
        for name, t in folded.items():
            t = _f32(t.detach().to(torch.float32).contiguous())
            check(lib().gvc_hifigan_bind_weight(self._h, name.encode(), ptr(t), t.numel(), stream()), f"bind {name}")
        torch.cuda.current_stream().synchronize()
        missing = lib().gvc_hifigan_missing_weights(self._h)
        if missing:
            raise _lib.GenvcHipError(f"{missing} HiFi-GAN weight tensors missing after bind")

    def forward(self, x):
        """x [B,in_dim,T] -> [B,1,T*256]"""
        B, _, T = x.shape
        wav = torch.empty(B, 1, T * self.total_up, device=x.device, dtype=torch.float32)
        check(lib().gvc_hifigan_forward(self._h, ptr(_f32(x)), B, T, ptr(wav), stream()), "hifigan_forward")
        return wav

    def forward_latents(self, latents, scale=4):
        """latents [B,n,in_dim] -> [B,1,n*scale*256]  (F.interpolate(scale, 'linear') fused in front)"""
        B, n, _ = latents.shape
        wav = torch.empty(B, 1, n * scale * self.total_up, device=latents.device, dtype=torch.float32)
        check(lib().gvc_hifigan_forward_latents(self._h, ptr(_f32(latents)), B, n, scale, ptr(wav), stream()),
              "hifigan_forward_latents")
        return wav


def mpd_channels(mult):
    """DiscriminatorP's channel widths (reference layers/hifigan.py:327-363: int(32 m), int(128 m), int(512 m), int(1024 m) twice)"""
    return [int(32 * mult), int(128 * mult), int(512 * mult), int(1024 * mult), int(1024 * mult)]


class DiscriminatorEngine:
    """MultiScaleDiscriminator / MultiPeriodDiscriminator.forward in eval mode (reference layers/hifigan.py:281-314, :399-426) with
    the reductions of the criteria (layers/hifigan_loss.py:78-123) in the same call.  fp32; the feature maps live in an arena
    tensor this object owns and are overwritten by the next forward."""

    def __init__(self, kind, periods=(), mult=1.0, spectral_norm=False, max_batch=2, max_samples=24000):
        if kind not in ("MSD", "MPD"):
            raise NotImplementedError(f"discriminator {kind!r} is not served (MSD and MPD are)")
        d = _lib.DiscDims()
        d.kind = _lib.DISC_MSD if kind == "MSD" else _lib.DISC_MPD
        self.kind, self.periods = kind, [int(p) for p in periods]
        if kind == "MPD":
            if not 1 <= len(self.periods) <= 8:
                raise ValueError(f"MPD: {len(self.periods)} periods (1..8 are supported)")
            d.n_sub = len(self.periods)
            for i, p in enumerate(self.periods):
                d.periods[i] = p
            for i, ch in enumerate(mpd_channels(mult)):
                d.channels[i] = ch
            d.spectral_norm = int(bool(spectral_norm))
        else:
            d.n_sub = 3
        d.max_batch, d.max_samples = max_batch, max_samples
        self.n_sub = d.n_sub
        self.max_batch, self.max_samples = max_batch, max_samples
        self._h = C.c_void_p()
        self._arena = None
        check(lib().gvc_disc_create(C.byref(d), C.byref(self._h)), "gvc_disc_create")
        self.n_layers = lib().gvc_disc_layers(self._h)
        self._arena = torch.empty(lib().gvc_disc_arena_floats(self._h), device="cuda", dtype=torch.float32)
        check(lib().gvc_disc_set_arena(self._h, ptr(self._arena)), "gvc_disc_set_arena")

    def close(self):
        if self._h:
            lib().gvc_disc_destroy(self._h)
            self._h = C.c_void_p()
        self._arena = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, weights, prefix=""):
        """weights: reference state dict (weight_g / weight_v / bias, or weight_orig / weight_u / weight_v / bias); both
        parametrisations are folded by the library"""
        for name, t in weights.items():
            if not name.startswith(prefix) or not torch.is_tensor(t) or not t.is_floating_point():
                continue
            t = _f32(t.detach().to(torch.float32).contiguous())
            check(lib().gvc_disc_bind_weight(self._h, name[len(prefix):].encode(), ptr(t), t.numel(), stream()), f"bind {name}")
        torch.cuda.current_stream().synchronize()
        missing = lib().gvc_disc_missing_weights(self._h)
        if missing:
            raise _lib.GenvcHipError(f"{missing} discriminator weight tensors missing after bind")

    def folded_weight(self, sub, layer, shape):
        out = torch.empty(*shape, device="cuda", dtype=torch.float32)
        check(lib().gvc_disc_folded_weight(self._h, sub, layer, ptr(out), out.numel(), stream()), "disc_folded_weight")
        return out

    def layer(self, sub, layer, B, T):
        """the feature map of one layer after a forward at (B, T): a view [2 B, C, H, W] of the arena"""
        off, c, h, w = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().gvc_disc_layer(self._h, sub, layer, B, T, C.byref(off), C.byref(c), C.byref(h), C.byref(w)), "disc_layer")
        n = 2 * B * c.value * h.value * w.value
        return self._arena[off.value:off.value + n].view(2 * B, c.value, h.value, w.value)

    def forward(self, y, y_hat):
        """y, y_hat [B,T] -> stats float32 [n_sub, 3 + n_layers]: mean((1 - d_r)^2), mean(d_g^2), mean((1 - d_g)^2), then
        mean|f_r - f_g| per layer; the feature maps are read with layer()"""
        B, T = y.shape
        if tuple(y_hat.shape) != (B, T):
            raise ValueError(f"discriminator: y {tuple(y.shape)} and y_hat {tuple(y_hat.shape)} differ in shape")
        stats = torch.empty(self.n_sub, 3 + self.n_layers, device=y.device, dtype=torch.float32)
        check(lib().gvc_disc_forward(self._h, ptr(_f32(y)), ptr(_f32(y_hat)), B, T, ptr(stats), stream()), "disc_forward")
        return stats


    def time_layer(self, sub, layer, B, T, iters=20):
        """microseconds per launch of one layer alone (measurement; run a forward at (B, T) first)"""
        us = C.c_float()
        check(lib().gvc_disc_time_layer(self._h, sub, layer, B, T, iters, C.byref(us), stream()), "disc_time_layer")
        return us.value


def l1_mean(a, b, scale=1.0):
    """scale * mean|a - b| as a 0-d device tensor, reduced in a fixed order (the same input gives the same bits)"""
    if a.shape != b.shape:
        raise ValueError(f"l1_mean: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    a, b = _f32(a), _f32(b)
    out = torch.empty(1, device=a.device, dtype=torch.float32)
    work = torch.empty(256, device=a.device, dtype=torch.float64)
    check(lib().gvc_l1_mean(ptr(a), ptr(b), a.numel(), float(scale), ptr(out), ptr(work), stream()), "l1_mean")
    return out[0]


class MelLossEngine:
    """extract_mel_features of the reference's layers/hifigan_loss.py:16-75: reflect padding of (fft_size - hop) / 2 with
    center=False, magnitude sqrt(re^2 + im^2 + 1e-9), librosa's default (Slaney) filterbank, log(clamp(., 1e-5))."""

    def __init__(self, sample_rate=24000, fft_size=1024, num_mels=100, mel_fmin=0, mel_fmax=12000, win_length=1024, hop_length=256):
        o = _lib.MelOptions()
        o.n_fft, o.hop, o.win, o.sample_rate, o.n_mels = fft_size, hop_length, win_length, sample_rate, num_mels
        o.flags = _lib.MEL_SLANEY_SCALE | _lib.MEL_MAGNITUDE | _lib.MEL_PAD_HALF_OVERLAP
        o.f_min, o.f_max = float(mel_fmin), float(mel_fmax if mel_fmax is not None else sample_rate / 2.0)
        self.n_mels, self.pad = num_mels, (fft_size - hop_length) // 2
        self._h = C.c_void_p()
        check(lib().gvc_mel_create_ex(C.byref(o), C.byref(self._h)), "gvc_mel_create_ex")

    def close(self):
        if self._h:
            lib().gvc_mel_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, wav):
        """wav [B,T] -> [B,n_mels,T // hop]; ValueError when T does not exceed the reflect padding"""
        B, T = wav.shape
        if T <= self.pad:
            raise ValueError(f"mel loss: {T} samples are too few for reflect padding of {self.pad}")
        nf = lib().gvc_mel_frames(self._h, T)
        out = torch.empty(B, self.n_mels, nf, device=wav.device, dtype=torch.float32)
        check(lib().gvc_mel_forward(self._h, ptr(_f32(wav)), B, T, ptr(out), None, stream()), "mel_forward")
        return out


class HubertEngine:
    """ContentVecExtractor.extract_content_features (reference layers/content_processor.py:17-31): HuBERT-base
    extract_features(output_layer=n_layers) + final_proj, weights under fairseq's names."""

    def __init__(self, cfg, max_batch=2, max_samples=16000 * 30):
        self.cfg = dict(cfg)
        d = _lib.HubertDims()
        d.n_conv = len(cfg["conv_layers"])
        for i, (c, k, s) in enumerate(cfg["conv_layers"]):
            d.conv_dim[i], d.conv_kernel[i], d.conv_stride[i] = c, k, s
        d.embed_dim, d.n_layers, d.n_heads, d.ffn_dim = cfg["embed_dim"], cfg["layers"], cfg["heads"], cfg["ffn_dim"]
        d.pos_conv_kernel, d.pos_conv_groups, d.final_dim = cfg["pos_conv_kernel"], cfg["pos_conv_groups"], cfg["final_dim"]
        d.max_batch, d.max_samples = max_batch, max_samples
        self.final_dim = cfg["final_dim"]
        self._h = C.c_void_p()
        check(lib().gvc_hubert_create(C.byref(d), C.byref(self._h)), "gvc_hubert_create")

    def close(self):
        if self._h:
            lib().gvc_hubert_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, weights, prefix=""):
        """weights: fairseq-named state dict; the weight-normed positional conv (weight_g, weight_v; dim=2) is
        folded here (loader plumbing, as torch's remove_weight_norm would)."""
        sd = {k[len(prefix):]: v for k, v in weights.items() if k.startswith(prefix) and torch.is_tensor(v)}
        pc = "encoder.pos_conv.0."
        if pc + "weight_v" in sd:
            v, g = sd.pop(pc + "weight_v").float(), sd.pop(pc + "weight_g").float()
            sd[pc + "weight"] = g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()
        for name, t in sd.items():
            if not t.is_floating_point():
                continue
            t = _f32(t.detach().to(torch.float32).contiguous())
            check(lib().gvc_hubert_bind_weight(self._h, name.encode(), ptr(t), t.numel(), stream()), f"bind {name}")
        torch.cuda.current_stream().synchronize()
        missing = lib().gvc_hubert_missing_weights(self._h)
        if missing:
            raise _lib.GenvcHipError(f"{missing} HuBERT weight tensors missing after bind")

    def frames(self, n_samples):
        return lib().gvc_hubert_frames(self._h, int(n_samples))

    def forward(self, wav):
        """wav [B,T] 16 kHz -> [B,T50,final_dim]"""
        B, T = wav.shape
        n = self.frames(T)
        if n < 1:
            raise ValueError(f"{T} samples are too short for the HuBERT conv stack")
        out = torch.empty(B, n, self.final_dim, device=wav.device, dtype=torch.float32)
        check(lib().gvc_hubert_forward(self._h, ptr(_f32(wav)), B, T, ptr(out), stream()), "hubert_forward")
        return out


def resample(wav, orig_sr, new_sr):
    """wav [B,T] (CUDA) -> [B, ceil(T*new/orig)]: torchaudio.functional.resample defaults (reference utils.py:58-62)"""
    B, T = wav.shape
    n = lib().gvc_resample_length(T, int(orig_sr), int(new_sr))
    out = torch.empty(B, n, device=wav.device, dtype=torch.float32)
    check(lib().gvc_resample(ptr(_f32(wav)), B, T, int(orig_sr), int(new_sr), ptr(out), stream()), "resample")
    return out
