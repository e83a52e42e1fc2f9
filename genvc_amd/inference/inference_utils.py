"""Inference harness with the reference's function names and semantics
(/root/reference/inference/inference_utils.py): segmentation (:34-50), per-segment independence,
stop-token stripping (:68), streaming groups of `stream_chunk_size` tokens with the EOS-step latent
included (:187-207), cross-fade of vocoder chunks (:4-21), latency / RTF bookkeeping (:148, 208-216).

The vocoder call (x4 linear interpolation + HiFi-GAN) runs on libgenvc_hip; when
`model.hifigan` is None the functions return the acoustic latents instead of a waveform.
"""
import time

import torch
import torch.nn.functional as F


@torch.inference_mode()
def handle_chunks(wav_gen, wav_gen_prev, wav_overlap, overlap_len=1024):
    """reference :4-21"""
    wav_chunk = wav_gen[:-overlap_len]
    if wav_overlap is not None:
        if overlap_len > len(wav_chunk):
            return wav_gen[-overlap_len:], wav_gen, None
        fade_in = wav_chunk[:overlap_len] * torch.linspace(0.0, 1.0, overlap_len, device=wav_chunk.device)
        wav_chunk[:overlap_len] = wav_overlap * torch.linspace(1.0, 0.0, overlap_len, device=wav_overlap.device)
        wav_chunk[:overlap_len] += fade_in
    return wav_chunk, wav_gen, wav_gen[-overlap_len:]


def segments(src_wav, seg_len, min_len):
    """reference :43-50: fixed-length segments, the last one zero-padded to at least 0.32 s"""
    total = src_wav.shape[-1]
    for i in range(0, total, seg_len):
        if i + seg_len >= total:
            seg = src_wav[:, i:]
            if seg.shape[-1] < min_len:
                seg = F.pad(seg, (0, min_len - seg.shape[-1]), "constant", 0)
        else:
            seg = src_wav[:, i:i + seg_len]
        yield seg


def _sampling_kwargs(model):
    c = model.config
    return dict(top_p=c.top_p, top_k=c.top_k, temperature=c.temperature, length_penalty=c.length_penalty,
                repetition_penalty=c.repetition_penalty, do_sample=True, num_beams=1)


def _vocode(model, latents):
    """latents [1,n,d] -> waveform: F.interpolate(scale_factor=hifigan_scale_factor, mode='linear') + HiFi-GAN
    (reference :81-87, :196-202); both run inside one library call.  None without a vocoder."""
    if model.hifigan is None:
        return None
    scale = int(model.hifigan_scale_factor)
    if hasattr(model.hifigan, "forward_latents") and scale == model.hifigan_scale_factor:
        return model.hifigan.forward_latents(latents, scale)
    mel_input = F.interpolate(latents.transpose(1, 2), scale_factor=[model.hifigan_scale_factor], mode="linear").squeeze(1)
    return model.hifigan(mel_input)


@torch.inference_mode()
def negative_cond_latents(m, guidance_scale, negative_ref_audio, src_wav):
    """the unconditional prompt's conditioning latents of a guided conversion (GPT.generate(guidance_scale=...,
    negative_cond_latents=...)), or None when guidance is off.  negative_ref_audio: (wav [1, T], sample rate) of the negative speaker,
    default the source utterance itself (src_wav at the content sample rate) -- the speaker whose timbre leaks; it goes through
    get_gpt_cond_latents as the target reference does, resampled to the conditioning sample rate when it comes at another."""
    from genvc_amd.layers.gpt import _guidance_scale
    if _guidance_scale({"guidance_scale": guidance_scale}) is None:
        return None
    wav, sr = negative_ref_audio if negative_ref_audio is not None else (src_wav, m.content_sample_rate)
    wav = wav.to(m.device)
    if wav.ndim == 1:
        wav = wav[None]
    target = int(m.config.audio.sample_rate)
    if int(sr) != target:
        from genvc_amd.engine import resample
        wav = resample(wav.to(torch.float32).contiguous(), int(sr), target)
    return m.get_gpt_cond_latents(wav, target)


def _guided_kwargs(m, gkw, guidance_scale, negative_ref_audio, src_wav):
    """gkw with guidance_scale / negative_cond_latents of a guided conversion merged in (the negative latents computed here, once per
    utterance, unless the caller's generate_kwargs already carry them); gkw itself when guidance is off"""
    if guidance_scale is None:
        guidance_scale = gkw.get("guidance_scale")
    neg = gkw.get("negative_cond_latents")
    if neg is None:
        neg = negative_cond_latents(m, guidance_scale, negative_ref_audio, src_wav)
    if neg is None:
        return gkw if guidance_scale is None else dict(gkw, guidance_scale=guidance_scale)
    return dict(gkw, guidance_scale=guidance_scale, negative_cond_latents=neg)


@torch.inference_mode()
def _segment_latents(m, cond_latent, codes, gen, repass_latents, row=0):
    """the acoustic latents of one segment's n non-stop tokens.  The reference recomputes them with a second, teacher-forced forward pass
    over [cond | codes | start, gen, stop x 4] and trims it with `sub = -5` (inference_utils.py:71-76, gpt.py:375-508, :491, :508); row i of
    that pass is the hidden state that predicted token i -- the very vector the decode loop already produced at step i
    (stream_generator.py:865; SURVEY.md 8a row 12: equal to <= 4.8e-7).  Default: reuse the decode-time latents of `GPT.generate`
    (`last_latents`, the EOS-step latent dropped: the re-pass has n rows); `repass_latents=True` runs the reference's second pass.
    row: the row of the generate call `gen` came from (a candidate of generate(num_return_sequences=N))."""
    n = int(gen.shape[-1])
    if not repass_latents and getattr(m.gpt, "last_latents", None) is not None and m.gpt.last_latents.shape[1] >= n:
        return m.gpt.last_latents[row:row + 1, :n]
    out_len = torch.tensor([n * m.config.model_args.gpt_code_stride_len], device=m.device)
    clen = torch.tensor([codes.shape[-1]], device=m.device)
    return m.gpt(codes, clen, gen.unsqueeze(0), out_len, cond_latents=cond_latent, return_latent=True)


@torch.inference_mode()
def synthesize_utt(genVC_mdl, src_wav, tgt_audio, seg_len=6.0, return_details=False, repass_latents=False, num_beams=1,
                   generate_kwargs=None, num_return_sequences=None, num_beam_groups=None, diversity_penalty=None, guidance_scale=None,
                   negative_ref_audio=None, token_scores=False, alignment=False):
    """non-streaming conversion, latent-level concatenation (reference :23-89).  num_beams = K > 1: every segment decodes with
    deterministic beam search (GPT.generate(num_beams=K, do_sample=False)); its latents come from the re-pass.
    generate_kwargs: more GPT.generate kwargs (the logits processors: min_new_tokens, no_repeat_ngram_size, ...; the
    sampling warpers typical_p, epsilon_cutoff, eta_cutoff; ras_window / ras_threshold; presence_penalty, frequency_penalty,
    penalty_window), merged into every segment's call (synthesize_utt_chunked passes them on likewise).
    num_return_sequences = N > 1 (the keyword, or in generate_kwargs): a LIST of N results, candidate j of the utterance being the
    concatenation of candidate j of every segment (GPT.generate(num_return_sequences=N) per segment: one prefill, N rows); with
    return_details each dict also carries "score", the sum over the segments of the candidate's score (sampling: sequence_logprobs,
    the raw model distribution; beam search: the normalised beam score).
    num_beam_groups = G > 1 with diversity_penalty > 0 (the keywords, or in generate_kwargs; needs num_beams = K, a multiple of G):
    every segment decodes with group (diverse) beam search, whose N best hypotheses start from different groups.
    guidance_scale = s != 1 (the keyword, or in generate_kwargs): classifier-free guidance (GPT.generate(guidance_scale=s)): every segment
    decodes under the target reference and under a negative speaker, negative_ref_audio = (wav, sample rate), default the source
    utterance itself; its conditioning latents are computed once for the utterance.
    token_scores=True with return_details: the dict also carries "token_logprobs", one fp32 [n] tensor per segment beside "codes": the
    log-probability of every token under the distribution it was decoded from (GPT.generate(output_scores=True) and
    compute_transition_scores(normalize_logits=True): processors, warpers and guidance included).  Not with num_return_sequences > 1;
    beams and contrastive search raise NotImplementedError (GPT.generate).
    alignment=True with return_details: the dict also carries "alignments", one fp32 [n, Tc] matrix per segment beside "codes": the
    attention of each of the segment's n acoustic codes over its Tc content codes (GPT.trace(output_attentions=False): the head /
    layer mean, one more teacher-forced pass per segment; a row sums to at most 1).  Not with num_return_sequences > 1."""
    m = genVC_mdl
    from genvc_amd.layers.gpt import _num_return
    if alignment and not return_details:
        raise ValueError("alignment=True needs return_details=True (the matrices come back in the details dict)")
    if token_scores and not return_details:
        raise ValueError("token_scores=True needs return_details=True (the scores come back in the details dict)")
    gkw = dict(generate_kwargs or {})
    if num_return_sequences is not None:
        gkw["num_return_sequences"] = num_return_sequences
    if num_beam_groups is not None:
        gkw["num_beam_groups"] = num_beam_groups
    if diversity_penalty is not None:
        gkw["diversity_penalty"] = diversity_penalty
    gkw = _guided_kwargs(m, gkw, guidance_scale, negative_ref_audio, src_wav)
    if token_scores and _num_return(gkw) > 1:
        raise NotImplementedError("token_scores=True with num_return_sequences > 1 is not implemented: the candidates carry "
                                  "their sequence scores")
    if alignment and _num_return(gkw) > 1:
        raise NotImplementedError("alignment=True with num_return_sequences > 1 is not implemented: GPT.trace serves each candidate's codes")
    if token_scores:
        gkw.update(return_dict_in_generate=True, output_scores=True)
    if _num_return(gkw) > 1:
        return _synthesize_candidates(m, src_wav, tgt_audio, seg_len, return_details, repass_latents, num_beams, gkw)
    min_len = int(0.32 * m.content_sample_rate)
    src_wav = src_wav.to(m.device)
    seg = int(seg_len * m.content_sample_rate)
    cond_latent = m.get_gpt_cond_latents(tgt_audio.to(m.device), m.config.audio.sample_rate)
    final_latents, all_codes, all_logprobs, all_aligns = [], [], [], []
    more = {"token_logprobs": all_logprobs} if token_scores else {}
    if alignment:
        more["alignments"] = all_aligns
    ras = return_details and gkw.get("ras_window")       # (details only: reading the counters waits for the segment)
    if ras:
        more["ras_redraws"] = []
    for src_seg in segments(src_wav, seg, min_len):
        feat = m.content_extractor.extract_content_features(src_seg)
        codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
        kw = _sampling_kwargs(m) if num_beams == 1 else dict(_sampling_kwargs(m), do_sample=False, num_beams=int(num_beams))
        res = m.gpt.generate(cond_latent, codes, output_attentions=False, **dict(kw, **gkw))
        gen = getattr(res, "sequences", res)[0]          # (a caller's own return_dict_in_generate in generate_kwargs: the tokens of the result)
        if ras and m.gpt.last_ras_redraws is not None:
            more["ras_redraws"].append(int(m.gpt.last_ras_redraws.sum()))
        keep = gen != m.gpt.stop_audio_token
        gen = gen[keep]                                                 # reference :68 (0-d collapse guarded)
        if gen.numel() == 0:
            continue
        final_latents.append(_segment_latents(m, cond_latent, codes, gen, repass_latents))
        all_codes.append(gen)
        if token_scores:
            all_logprobs.append(m.gpt.compute_transition_scores(res.sequences, res.scores, normalize_logits=True)[0][keep])
        if alignment:
            all_aligns.append(m.gpt.trace(cond_latent, codes, gen.unsqueeze(0), output_attentions=False).alignment[0])
    if not final_latents:                    # every segment ended on its first token: nothing to vocode
        empty = torch.zeros(0, device=m.device)
        return dict(latents=None, codes=[], wav=empty, **more) if return_details else empty
    latents = torch.cat(final_latents, dim=1)
    wav = _vocode(m, latents)
    if return_details or wav is None:
        return dict(latents=latents, codes=all_codes, wav=None if wav is None else wav[0].squeeze(), **more)
    return wav[0].squeeze()


def _synthesize_candidates(m, src_wav, tgt_audio, seg_len, return_details, repass_latents, num_beams, gkw):
    """synthesize_utt for num_return_sequences = N > 1 (gkw carries it)"""
    N = int(gkw["num_return_sequences"])
    min_len = int(0.32 * m.content_sample_rate)
    src_wav = src_wav.to(m.device)
    seg = int(seg_len * m.content_sample_rate)
    cond_latent = m.get_gpt_cond_latents(tgt_audio.to(m.device), m.config.audio.sample_rate)
    lats, codes_out, score = [[] for _ in range(N)], [[] for _ in range(N)], [0.0] * N
    kw = _sampling_kwargs(m) if num_beams == 1 else dict(_sampling_kwargs(m), do_sample=False, num_beams=int(num_beams))
    for src_seg in segments(src_wav, seg, min_len):
        feat = m.content_extractor.extract_content_features(src_seg)
        codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
        rows = m.gpt.generate(cond_latent, codes, output_attentions=False, **dict(kw, **gkw))
        rows = getattr(rows, "sequences", rows)
        sc = m.gpt.last_sequence_logprobs if m.gpt.last_latents is not None else m.gpt.last_beam_scores
        for j in range(N):
            score[j] += float(sc[j])
            gen = rows[j][rows[j] != m.gpt.stop_audio_token]
            if gen.numel() == 0:
                continue
            lats[j].append(_segment_latents(m, cond_latent, codes, gen, repass_latents, row=j))
            codes_out[j].append(gen)
    out = []
    for j in range(N):
        if not lats[j]:
            empty = torch.zeros(0, device=m.device)
            out.append(dict(latents=None, codes=[], wav=empty, score=score[j]) if return_details else empty)
            continue
        latents = torch.cat(lats[j], dim=1)
        wav = _vocode(m, latents)
        if return_details or wav is None:
            out.append(dict(latents=latents, codes=codes_out[j], wav=None if wav is None else wav[0].squeeze(), score=score[j]))
        else:
            out.append(wav[0].squeeze())
    return out


@torch.inference_mode()
def synthesize_utt_chunked(genVC_mdl, src_wav, tgt_audio, seg_len=6.0, repass_latents=False, generate_kwargs=None, guidance_scale=None,
                           negative_ref_audio=None):
    """non-streaming conversion with waveform-level concatenation (reference :92-133): every segment goes through
    `genVC_mdl.inference` (trainers/hifigan_trainer.py:457-500) and the segment waveforms are joined by `handle_chunks`
    (1024 samples dropped from each, cross-fade over the previous tail).  generate_kwargs, guidance_scale, negative_ref_audio: as
    synthesize_utt (the negative latents are computed once here and handed to every segment's `inference` call)"""
    m = genVC_mdl
    from genvc_amd.layers.gpt import _single_return
    _single_return(generate_kwargs or {}, "chunked (synthesize_utt_chunked)")      # (it cross-fades ONE waveform per segment)
    generate_kwargs = _guided_kwargs(m, dict(generate_kwargs or {}), guidance_scale, negative_ref_audio, src_wav)
    wav_gen_prev, wav_overlap = None, None
    pred_audios = []
    min_len = int(0.32 * m.content_sample_rate)
    src_wav = src_wav.to(m.device)
    seg = int(seg_len * m.content_sample_rate)
    cond_latent = m.get_gpt_cond_latents(tgt_audio.to(m.device), m.config.audio.sample_rate)
    c = m.config
    for src_seg in segments(src_wav, seg, min_len):
        audio_pred = m.inference(src_seg, cond_latent, top_p=c.top_p, top_k=c.top_k, temperature=c.temperature,
                                 length_penalty=c.length_penalty, repetition_penalty=c.repetition_penalty, repass_latents=repass_latents,
                                 **({"generate_kwargs": generate_kwargs} if generate_kwargs else {}))
        wav_chunk, wav_gen_prev, wav_overlap = handle_chunks(audio_pred.squeeze(), wav_gen_prev, wav_overlap, 1024)
        pred_audios.append(wav_chunk)
    return torch.cat(pred_audios, dim=-1)


@torch.inference_mode()
def synthesize_utt_streaming(genVC_mdl, src_wav, tgt_audio, seg_len=6.0, stream_chunk_size=8, verbose=True,
                             return_details=False, generate_kwargs=None):
    """streaming conversion (reference :135-217); the clock starts before the host->device copies (:148).  generate_kwargs: more
    GPT.get_generator kwargs (the logits processors, ras_window / ras_threshold, presence_penalty / frequency_penalty /
    penalty_window), merged into every segment's call; with ras_window
    the details carry "ras_redraws", the redraws of every segment.  sequence_bias / bad_words_ids /
    forced_eos_token_id / renormalize_logits and assistant_model raise NotImplementedError here (infer.py --streaming): synthesize_utt
    serves them"""
    from genvc_amd.layers.gpt import _no_assistant, _no_bias
    _no_bias(generate_kwargs or {}, "the streaming (synthesize_utt_streaming, infer.py --streaming) path")
    _no_assistant(generate_kwargs or {}, "streaming (synthesize_utt_streaming, infer.py --streaming)")
    m = genVC_mdl
    wav_gen_prev, wav_overlap = None, None
    total = src_wav.shape[-1]
    pred, chunks_lat, tokens = [], [], []
    ras_redraws = []
    min_len = int(0.32 * m.content_sample_rate)
    begin = time.time()
    latency = None
    src_wav = src_wav.to(m.device)
    seg = int(seg_len * m.content_sample_rate)
    # the reference computes the conditioning latents first (:152-153); they do not depend on the source, so here their mel + Perceiver
    # chain runs on a second stream beside the first segment's ContentVec + DVAE chain (same arithmetic, shorter first-chunk latency)
    # -- and its ~25 launches are enqueued AFTER the first segment's ContentVec + DVAE launches (the side stream only waits for the uploads):
    # the GPU starts on the source while the host is still busy with the conditioning chain
    tgt_dev = tgt_audio.to(m.device)
    can_async = hasattr(m, "get_gpt_cond_latents_async")
    uploaded = torch.cuda.Event() if can_async else None
    if uploaded is not None:
        uploaded.record()
    cond_future = None
    cond_latent = None if can_async else m.get_gpt_cond_latents(tgt_dev, m.config.audio.sample_rate)
    cached = 0          # prefix caching: after the first segment the conditioning rows are already in the KV cache
    for src_seg in segments(src_wav, seg, min_len):
        feat = m.content_extractor.extract_content_features(src_seg)
        codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
        if cond_latent is None:
            if cond_future is None:
                cond_future = m.get_gpt_cond_latents_async(tgt_dev, m.config.audio.sample_rate, after=uploaded)
            cond_latent = cond_future.result()
        fake = m.gpt.compute_embeddings(cond_latent, codes)
        gen = m.gpt.get_generator(fake_inputs=fake, num_return_sequences=1, output_attentions=False,
                                  output_hidden_states=True, stream_group=max(stream_chunk_size, 1),
                                  cached_cond_rows=cached, **dict(_sampling_kwargs(m), **(generate_kwargs or {})))
        cached = cond_latent.shape[1]
        last_tokens, all_latents = [], []
        is_end = False
        while not is_end:
            try:
                x, latent = next(gen)
                last_tokens.append(x)
                all_latents.append(latent)
            except StopIteration:
                is_end = True
            # DIVERGENCE from the reference, on purpose: inference_utils.py:192-196 runs `torch.cat(all_latents)` whenever `is_end` is
            # set, so a segment whose token count is a multiple of stream_chunk_size (the last group was flushed by the count rule,
            # then StopIteration arrives with nothing pending) crashes there on torch.cat([]).  Here an empty tail is skipped.
            if (is_end and all_latents) or (stream_chunk_size > 0 and len(last_tokens) >= stream_chunk_size):
                acoustic = torch.cat(all_latents, dim=0)[None, :]       # EOS-step latent included (:189-196)
                chunks_lat.append(acoustic)
                tokens.append(torch.stack(last_tokens, 1))
                audio = _vocode(m, acoustic)
                if audio is not None:
                    wav_chunk, wav_gen_prev, wav_overlap = handle_chunks(audio.squeeze(), wav_gen_prev, wav_overlap, 1024)
                    pred.append(wav_chunk)
                last_tokens, all_latents = [], []
                if latency is None:
                    torch.cuda.synchronize()
                    latency = time.time() - begin
                    if verbose:
                        print(f"Latency: {latency:.3f}s")
        if return_details and m.gpt.last_ras_redraws is not None and (generate_kwargs or {}).get("ras_window"):
            ras_redraws.append(int(m.gpt.last_ras_redraws.sum()))
    if cond_latent is None and cond_future is not None:
        cond_future.result()          # no segment consumed the latents: still join the side stream (its scratch buffers are per context)
    torch.cuda.synchronize()
    rtf = (time.time() - begin) / (total / m.content_sample_rate)
    if verbose:
        print(f"Real-time factor: {rtf:.3f}")
    if return_details or not pred:
        more = {"ras_redraws": ras_redraws} if (generate_kwargs or {}).get("ras_window") else {}
        return dict(wav=torch.cat(pred, -1) if pred else None, latents=chunks_lat, tokens=tokens, latency=latency, rtf=rtf, **more)
    return torch.cat(pred, dim=-1)


@torch.inference_mode()
def synthesize_streams_streaming(genVC_mdl, src_wavs, tgt_audios, seg_len=1.0, stream_chunk_size=8, return_details=True,
                                 generate_kwargs=None):
    """BASELINE configs[3]: B concurrent streams stepped together.  Each stream is converted exactly as
    `synthesize_utt_streaming` converts it on its own (same segments, same per-stream EOS rule, same vocoder grouping and
    cross-fade); the streams only SHARE the launches: ContentVec / DVAE / prefill / vocoder run on the batch and one
    decode step serves every stream (the MFMA rows path from 5 streams up).

    src_wavs [B,T] (equal lengths), tgt_audios [B,Tr] or [1,Tr] (one reference for all).
    generate_kwargs: more GPT.get_generator kwargs for every stream (the logits processors, ras_window / ras_threshold,
    presence_penalty / frequency_penalty / penalty_window); with
    ras_window the result carries "ras_redraws", per stream the redraws of its segments.
    Returns per-stream lists: wav [B] tensors, tokens, plus first-chunk latency and the batch RTF."""
    from genvc_amd.layers.gpt import _no_assistant, _no_bias
    _no_bias(generate_kwargs or {}, "the streaming (synthesize_streams_streaming) path")
    _no_assistant(generate_kwargs or {}, "streaming (synthesize_streams_streaming)")
    m = genVC_mdl
    B, total = src_wavs.shape
    min_len = int(0.32 * m.content_sample_rate)
    begin = time.time()
    latency = None
    src_wavs = src_wavs.to(m.device)
    seg = int(seg_len * m.content_sample_rate)
    sr = m.config.audio.sample_rate
    tgt = tgt_audios.to(m.device)
    conds = [m.get_gpt_cond_latents(tgt[i:i + 1], sr) for i in range(tgt.shape[0])]
    cond_latent = torch.cat(conds if len(conds) == B else conds * B, 0)
    stop = m.gpt.stop_audio_token
    prev, overlap = [None] * B, [None] * B
    pred, tokens = [[] for _ in range(B)], [[] for _ in range(B)]
    ras_redraws = [[] for _ in range(B)]
    cached = 0
    for src_seg in segments(src_wavs, seg, min_len):
        feat = m.content_extractor.extract_content_features(src_seg)
        codes = m.content_dvae.get_codebook_indices(feat.transpose(1, 2))
        fake = m.gpt.compute_embeddings(cond_latent, codes)
        gen = m.gpt.get_generator(fake_inputs=fake, num_return_sequences=1, output_attentions=False,
                                  output_hidden_states=True, stream_group=max(stream_chunk_size, 1),
                                  cached_cond_rows=cached, **dict(_sampling_kwargs(m), **(generate_kwargs or {})))
        cached = cond_latent.shape[1]
        alive = [True] * B                        # a stream stops with its own EOS step (latent included, :189-196)
        g_tok, g_lat = [], []
        is_end = False
        while not is_end:
            try:
                x, latent = next(gen)
                g_tok.append(x)
                g_lat.append(latent)
            except StopIteration:
                is_end = True
            if (is_end and g_tok) or (stream_chunk_size > 0 and len(g_tok) >= stream_chunk_size):
                toks = torch.stack(g_tok, 1)                                  # [B,n]
                lats = torch.stack(g_lat, 1)                                  # [B,n,d]
                toks_h = toks.cpu()
                keep = []
                for b in range(B):
                    nb = 0
                    if alive[b]:
                        row = toks_h[b]
                        hit = (row == stop).nonzero()
                        nb = int(hit[0]) + 1 if hit.numel() else row.shape[0]
                        if hit.numel():
                            alive[b] = False
                        tokens[b].append(toks[b:b + 1, :nb])
                    keep.append(nb)
                # streams with the same group length share one vocoder call
                for nb in sorted(set(k for k in keep if k > 0)):
                    idx = [b for b in range(B) if keep[b] == nb]
                    audio = _vocode(m, lats[idx, :nb].contiguous())
                    if audio is None:
                        continue
                    for j, b in enumerate(idx):
                        chunk, prev[b], overlap[b] = handle_chunks(audio[j].squeeze(), prev[b], overlap[b], 1024)
                        pred[b].append(chunk)
                g_tok, g_lat = [], []
                if latency is None:
                    torch.cuda.synchronize()
                    latency = time.time() - begin
        if m.gpt.last_ras_redraws is not None and (generate_kwargs or {}).get("ras_window"):
            for b, c in enumerate(m.gpt.last_ras_redraws.cpu().tolist()):
                ras_redraws[b].append(int(c))
    torch.cuda.synchronize()
    rtf = (time.time() - begin) / (total / m.content_sample_rate)
    more = {"ras_redraws": ras_redraws} if (generate_kwargs or {}).get("ras_window") else {}
    return dict(wav=[torch.cat(p, -1) if p else None for p in pred], tokens=tokens, latency=latency, rtf=rtf, **more)
