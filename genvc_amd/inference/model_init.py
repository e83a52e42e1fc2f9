"""`model_init(checkpoint_path, device) -> (model, config)` with the reference's contract
(/root/reference/inference/model_init.py:9-34): the checkpoint is `{'config': dict, 'model': state_dict}`
with keys prefixed `gpt.`, `content_dvae.`, `hifigan.`, `content_extractor.model.`, ...; it is loaded
non-strictly.  The container mirrors the attributes of `HiFiGANTrainer` that the inference harness uses
(trainers/hifigan_trainer.py:25-167, 438-455).  No coqpit: the config is a plain dict (genvc_amd.config).
"""
import torch
from torch import nn

from .. import config as gcfg
from ..engine import resample
from ..layers.content_processor import ContentvecExtractor
from ..layers.dvae import DiscreteVAE
from ..layers.gpt import GPT
from ..layers.hifigan import HiFiGAN
from ..utils import DEFAULT_MEL_NORM_FILE, TorchMelSpectrogram


class GenVCModel(nn.Module):
    """inference view of the reference's HiFiGANTrainer"""

    def __init__(self, config, content_extractor=None, hifigan=None):
        super().__init__()
        self.config = config
        a = config.model_args
        self.gpt = GPT(layers=a.gpt_layers, model_dim=a.gpt_n_model_channels, heads=a.gpt_n_heads,
                       max_text_tokens=a.gpt_max_text_tokens, max_mel_tokens=a.gpt_max_audio_tokens,
                       max_prompt_tokens=a.gpt_max_prompt_tokens, number_text_tokens=a.gpt_number_text_tokens,
                       start_text_token=a.gpt_start_text_token, stop_text_token=a.gpt_stop_text_token,
                       num_audio_tokens=a.gpt_num_audio_tokens, start_audio_token=a.gpt_start_audio_token,
                       stop_audio_token=a.gpt_stop_audio_token, code_stride_len=a.gpt_code_stride_len)
        c = config.content_dvae_config
        self.content_dvae = DiscreteVAE(channels=c.num_channels, normalization=None, positional_dims=1,
                                        num_tokens=c.num_tokens, codebook_dim=c.codebook_dim, hidden_dim=c.hidden_dim,
                                        num_resnet_blocks=c.num_resnet_blocks, kernel_size=c.kernel_size,
                                        num_layers=c.num_layers, use_transposed_convs=False)
        # hifigan_trainer.py:146 reads config.content_dvae_config.audio.dvae_sample_rate
        self.content_sample_rate = (c.get("audio") or {}).get("dvae_sample_rate", c.get("dvae_sample_rate", 16000))
        # ContentVec = HuBERT-base under fairseq's parameter names (hifigan_trainer.py:85); another extractor with
        # the same interface can be passed in
        self.content_extractor = content_extractor or ContentvecExtractor(config.get("hubert_config"))
        v = config.get("vocoder_config")
        if hifigan is None and v is not None:                             # hifigan_trainer.py:47-55
            # the reference's config spells the field `upsample_kernal_sizes` (configs/vocoder_configs.py:19, hifigan_trainer.py:53)
            up_kernels = v.get("upsample_kernal_sizes", v.get("upsample_kernel_sizes"))
            hifigan = HiFiGAN(v.input_feat_dim, v.upsample_initial_channel, v.resblock_kernel_sizes,
                              v.resblock_dilation_sizes, v.upsample_rates, up_kernels,
                              resblock_type=v.get("resblock_type", "2"))
        self.hifigan = hifigan
        self.hifigan_scale_factor = a.gpt_code_stride_len / (v.get("hop_length", 256) if v is not None else 256)  # :56
        self.torch_mel_spectrogram_style_encoder = TorchMelSpectrogram(
            filter_length=2048, hop_length=256, win_length=1024, normalize=False,
            sampling_rate=config.audio.sample_rate, mel_fmin=0, mel_fmax=8000, n_mel_channels=80,
            mel_norm_file=a.get("mel_norm_file") or DEFAULT_MEL_NORM_FILE)
        # the acoustic DVAE (trainers/gpt_trainer.py:73-99) only when the config carries one (a reference checkpoint's does;
        # default_config(with_acoustic=True)).  Its engine is bound on first use: a model that never tokenises audio allocates nothing
        ac = config.get("acoustic_dvae_config")
        self.acoustic_dvae = None
        if ac is not None:
            self.acoustic_dvae = DiscreteVAE(channels=ac.num_channels, normalization=None, positional_dims=1, num_tokens=ac.num_tokens,
                                             codebook_dim=ac.codebook_dim, hidden_dim=ac.hidden_dim,
                                             num_resnet_blocks=ac.num_resnet_blocks, kernel_size=ac.kernel_size,
                                             num_layers=ac.num_layers, use_transposed_convs=False, with_decoder=True)
            self.acoustic_sample_rate = (ac.get("audio") or {}).get("dvae_sample_rate",
                                                                     ac.get("dvae_sample_rate", config.audio.sample_rate))
            self.torch_mel_spectrogram_dvae = TorchMelSpectrogram(                      # gpt_trainer.py:97-99: the class defaults
                mel_norm_file=a.get("mel_norm_file") or DEFAULT_MEL_NORM_FILE, sampling_rate=self.acoustic_sample_rate)
        self._device = torch.device("cpu")

    @torch.inference_mode()
    def format_batch_on_device(self, batch):
        """reference trainers/gpt_trainer.py:198-254: {"wav" [B,1,T] at config.audio.sample_rate, "wav_lengths", "conditioning"
        [B,n_cond,1,Tc], "cond_lens", "text_lengths" (optional)} gains `cond_mels` [B,n_cond,80,.] (2048-point extractor),
        `audio_codes` (1024-point mel -> acoustic DVAE) and `text_inputs` (resample to the content rate, right-pad
        int(text_frame_rate * content_sample_rate) zero samples, ContentVec, content DVAE).  `text_lengths` defaults to the dataset's
        rule (dataset.py:56,154)."""
        if self.acoustic_dvae is None:
            raise NotImplementedError("format_batch_on_device: the config has no acoustic_dvae_config (default_config(with_acoustic=True))")
        sr = int(self.config.audio.sample_rate)
        if int(self.acoustic_sample_rate) != sr:
            raise NotImplementedError(f"format_batch_on_device: an acoustic DVAE at {self.acoustic_sample_rate} Hz for audio at {sr} Hz "
                                      "needs the reference's Kaiser-window resampler, which is not implemented")
        dev = self.device
        tfr = float(self.config.get("text_frame_rate", 0.02))
        cond = batch["conditioning"]
        B, n_cond, C, Tc = cond.shape
        mel = self.torch_mel_spectrogram_style_encoder(cond.reshape(B * n_cond, C, Tc).to(dev))
        batch["cond_mels"] = mel.view(B, n_cond, mel.shape[1], mel.shape[2])
        wav = batch["wav"].to(dev)
        batch["audio_codes"] = self.acoustic_dvae.get_codebook_indices(self.torch_mel_spectrogram_dvae(wav))
        content = wav.reshape(B, -1).to(torch.float32).contiguous()
        if sr != int(self.content_sample_rate):
            content = resample(content, sr, int(self.content_sample_rate))
        content = torch.nn.functional.pad(content, (0, content_pad_samples(tfr, self.content_sample_rate)))
        feat = self.content_extractor.extract_content_features(content)
        batch["text_inputs"] = self.content_dvae.get_codebook_indices(feat.transpose(1, 2))
        if batch.get("text_lengths") is None:
            batch["text_lengths"] = default_text_lengths(batch["wav_lengths"], sr, tfr)
        batch["text_lengths"] = torch.as_tensor(batch["text_lengths"]).to(torch.long)
        return batch

    @torch.inference_mode()
    def detect_watermark(self, codes=None, wav=None, sr=None, watermarking_config=None, lens=None, z_threshold=3.0,
                         ignore_repeated_ngrams=False, return_dict=True):
        """engine.WatermarkDetector on generated codes: `codes` [B, n] (or [n]) as GPT.generate returns them -- give `lens` when rows
        end in stop codes that should not count -- or, as a convenience, `wav` [B, T] / [B, 1, T] at `sr` (default and only served
        rate: config.audio.sample_rate): the codes the acoustic DVAE assigns to it, format_batch_on_device's `audio_codes`.
        watermarking_config: the one the codes were generated with (the key is the secret).  -> WatermarkDetector's result.
        The `wav` form is exactly score(audio_codes(wav)).  Whether a mark SURVIVES vocoder -> waveform -> tokeniser is a property of
        trained weights; no checkpoint was available to this project, so nobody has measured it: treat a negative result on audio
        as no evidence, and a positive one with the caution any unmeasured detector deserves.  The codes form has no such caveat."""
        from genvc_amd.engine import WatermarkDetector
        if (codes is None) == (wav is None):
            raise ValueError("detect_watermark: pass codes=... or wav=..., not both and not neither")
        det = WatermarkDetector(watermarking_config, self.gpt.num_audio_tokens, ignore_repeated_ngrams=ignore_repeated_ngrams)
        if wav is not None:
            if self.acoustic_dvae is None:
                raise NotImplementedError("detect_watermark(wav=...): the config has no acoustic_dvae_config "
                                          "(default_config(with_acoustic=True))")
            rate = int(self.config.audio.sample_rate)
            if (sr is not None and int(sr) != rate) or int(self.acoustic_sample_rate) != rate:
                raise NotImplementedError(f"detect_watermark(wav=...): audio at {sr or rate} Hz for an acoustic DVAE at "
                                          f"{self.acoustic_sample_rate} Hz and a model at {rate} Hz needs a resampler this path does not have")
            wav = wav.to(self.device)
            if wav.ndim == 2:
                wav = wav[:, None]
            codes = self.acoustic_dvae.get_codebook_indices(self.torch_mel_spectrogram_dvae(wav))
        return det(codes, lens=lens, z_threshold=z_threshold, return_dict=return_dict)

    @torch.inference_mode()
    def audition_codes(self, audio_codes, n_iter=64, seed=0):
        """audio codes [B,n] -> waveform [B, hop (F - 1)] at the acoustic DVAE's rate, without the vocoder: the DVAE's decoded mel
        through TorchMelSpectrogram.invert (inverse mel scale, then Griffin-Lim from the seeded start).  Tells "the codes are bad" from
        "the vocoder is bad"."""
        if self.acoustic_dvae is None:
            raise NotImplementedError("audition_codes: the config has no acoustic_dvae_config (default_config(with_acoustic=True))")
        mel = self.acoustic_dvae.decode(audio_codes)[0]
        return self.torch_mel_spectrogram_dvae.invert(mel, n_iter=n_iter, seed=seed)

    @torch.inference_mode()
    def evaluate(self, batch):
        """the reference trainer's eval_step without its trainer (gpt_trainer.py:256-283): format_batch_on_device, then GPT.forward ->
        {loss_text_ce, loss_mel_ce, top10acc, loss}"""
        b = self.format_batch_on_device(batch)
        loss_text, loss_mel, acc, _ = self.gpt(b["text_inputs"], b["text_lengths"], b["audio_codes"], b["wav_lengths"],
                                               cond_mels=b["cond_mels"], cond_lens=b["cond_lens"])
        a = self.config.model_args
        # configs/genVC_configs.py:146-147
        loss = float(a.get("gpt_loss_text_ce_weight", 0.01)) * loss_text + float(a.get("gpt_loss_mel_ce_weight", 1.0)) * loss_mel
        return dict(loss_text_ce=loss_text, loss_mel_ce=loss_mel, top10acc=acc, loss=loss)

    @torch.inference_mode()
    def format_vocoder_batch_on_device(self, batch):
        """reference trainers/hifigan_trainer.py:268-344: format_batch_on_device, then `wav_lengths += gpt_code_stride_len // 2`,
        `mel_latents` [B,n,d] = GPT.forward(..., return_latent=True) and `wav` zero-padded or cut to n_codes * gpt_code_stride_len;
        the tensors only the GPT needed are dropped from the batch"""
        b = self.format_batch_on_device(batch)
        dev = self.device
        stride = int(self.config.model_args.gpt_code_stride_len)
        b["wav_lengths"] = torch.as_tensor(b["wav_lengths"]).to(dev) + stride // 2
        b["mel_latents"] = self.gpt(b["text_inputs"], b["text_lengths"], b["audio_codes"], b["wav_lengths"], cond_mels=b["cond_mels"],
                                    cond_lens=b["cond_lens"], return_latent=True)
        want = int(b["audio_codes"].shape[1]) * stride
        wav = b["wav"].to(dev)
        b["wav"] = torch.nn.functional.pad(wav, (0, max(0, want - wav.shape[-1])))[:, :, :want].contiguous()
        for k in ("cond_mels", "cond_lens", "audio_codes", "text_lengths", "text_inputs", "conditioning"):
            b.pop(k, None)
        return b

    SERVED_DISCRIMINATORS = ("MSD", "MPD")

    def _vocoder_discriminator(self, key):
        """the discriminators of hifigan_trainer.py:57-71 that this build serves, created on first use (under the state-dict prefix
        `hifigan_discriminator.{key}.`, as the trainer's ModuleDict names them) and put in eval mode"""
        if key in ("MSTFT", "MSCQT"):
            raise NotImplementedError(f"discriminator {key} is not served (MSD and MPD are): it needs a spectrogram / CQT front end "
                                      "and 2-D convolutions")
        if key not in self.SERVED_DISCRIMINATORS:
            raise NotImplementedError(f"unknown discriminator {key!r} (MSD and MPD are served)")
        if not hasattr(self, "hifigan_discriminator"):
            self.hifigan_discriminator = nn.ModuleDict()
        if key not in self.hifigan_discriminator:
            from ..layers.hifigan import MultiPeriodDiscriminator, MultiScaleDiscriminator
            v = self.config.get("vocoder_config") or {}
            d = MultiScaleDiscriminator() if key == "MSD" else MultiPeriodDiscriminator(
                v.get("mpd_reshapes", [2, 3, 5, 7, 11]), v.get("mpd_discriminator_channel_mult_factor", 1), v.get("mpd_use_spectral_norm", False))
            self.hifigan_discriminator[key] = d.to(self.device).eval()
        return self.hifigan_discriminator[key]

    @torch.inference_mode()
    def evaluate_vocoder(self, batch, discriminators=("MSD", "MPD"), return_audio=False):
        """the vocoder trainer's eval_step without its trainer (hifigan_trainer.py:346-385): format_vocoder_batch_on_device, the latents
        interpolated x hifigan_scale_factor, the generator, then per discriminator discriminator_criterion on (wav, generated) and the
        mel loss -> {"loss_disc", "mel_loss", "{key}_Discriminator_loss" per discriminator, "discriminators"} as Python floats.
        The reference's trainer sums FOUR discriminators into loss_disc (MSD, MPD, MSTFT, MSCQT); this build serves the two
        waveform-domain ones, "discriminators" names what the sum covers, and asking for "MSTFT" / "MSCQT" raises.
        return_audio=True adds "audio_gt" and "audio_pred" [B,1,T]."""
        from ..layers.hifigan_loss import discriminator_criterion, mel_criterion
        keys = tuple(discriminators)
        models = [self._vocoder_discriminator(k) for k in keys]
        if self.hifigan is None:
            raise NotImplementedError("evaluate_vocoder: the config has no vocoder_config")
        b = self.format_vocoder_batch_on_device(batch)
        audio_gt = b["wav"].to(torch.float32)
        audio_pred = self.hifigan.forward_latents(b["mel_latents"], int(self.hifigan_scale_factor))
        if audio_pred.shape != audio_gt.shape:
            raise ValueError(f"evaluate_vocoder: generated {tuple(audio_pred.shape)} against wav {tuple(audio_gt.shape)}")
        crit = discriminator_criterion()
        out, total = {}, 0.0
        for key, d in zip(keys, models):
            y_r, y_g, _, _ = d(audio_gt, audio_pred)
            loss, _, _ = crit(y_r, y_g)
            out[f"{key}_Discriminator_loss"] = float(loss)
            total = total + loss.cpu()
        if not hasattr(self, "_mel_criterion"):
            self._mel_criterion = mel_criterion(self.config.get("vocoder_config") or {})
        out["loss_disc"] = float(total)
        out["mel_loss"] = float(self._mel_criterion(audio_gt, audio_pred))
        out["discriminators"] = keys
        if return_audio:
            out["audio_gt"], out["audio_pred"] = audio_gt, audio_pred
        return out

    @property
    def device(self):
        return self._device

    def to(self, device):
        self._device = torch.device(device)
        return super().to(device)

    @torch.inference_mode()
    def get_gpt_cond_latents(self, audio, sr, length=30, chunk_length=6):
        """reference trainers/hifigan_trainer.py:438-455 -> [1, 32, d]"""
        # a conditioning chain started by get_gpt_cond_latents_async whose result() was never called (no segment, an exception)
        # may still be running on the side stream with the per-context mel / Perceiver scratch buffers: wait for it first
        side = getattr(self, "_cond_stream", None)
        if side is not None and audio.is_cuda and torch.cuda.current_stream(audio.device) != side:
            torch.cuda.current_stream(audio.device).wait_stream(side)
        embs = []
        if audio.shape[1] > sr * length:
            audio = audio[:, :sr * length]
        for i in range(0, audio.shape[1], sr * chunk_length):
            chunk = audio[:, i:i + sr * chunk_length]
            if chunk.size(-1) < sr * 0.33:
                continue
            # (the mel kernel also writes the frames-major copy the Perceiver reads: get_style_emb's permute(0, 2, 1).contiguous() is free)
            mel, mel_fm = self.torch_mel_spectrogram_style_encoder(chunk.to(self.device).contiguous(), frames_major=True)
            embs.append(self.gpt.get_style_emb(mel, None, frames_major=mel_fm))
        return torch.stack(embs).mean(dim=0).transpose(1, 2).contiguous()

    def get_gpt_cond_latents_async(self, audio, sr, length=30, chunk_length=6, after=None):
        """get_gpt_cond_latents on a second HIP stream: the reference speaker's mel + Perceiver chain (~25 short launches) does not
        depend on the source audio, so the streaming harness runs it BESIDE the first segment's ContentVec + DVAE chain instead of
        in front of it (first-chunk latency; the arithmetic and its order inside each chain are unchanged).  Returns a handle whose
        .result() makes the caller's current stream wait for the latents and returns them.
        `after` (a torch.cuda.Event on the caller's stream at which `audio` is ready): the side chain waits for THAT instead of for everything
        the caller's stream holds -- so a caller can enqueue its own first kernels (ContentVec of the first segment) BEFORE spending the
        ~0.3 ms of host time this chain's ~25 launches take, and the GPU is not idle meanwhile."""
        return _CondFuture(self, audio, sr, length, chunk_length, after)

    @torch.inference_mode()
    def warmup(self, seg_len=1.0, streams=1, ref_seconds=3.0, stream_chunk_size=8, top_k=None, max_new_tokens=None, num_beams=1,
               contrastive_top_k=None, num_return_sequences=1, num_beam_groups=1, guidance=False, ras_window=None, ras_threshold=None,
               presence_penalty=None, frequency_penalty=None, penalty_window=None, watermarking_config=None):
        """Everything the FIRST conversion of this shape would otherwise pay inside its latency window (the reference leaves warm-up
        to the user: /root/reference/infer.py:27-30 runs a conversion first).  For `streams` concurrent streams of `seg_len`-second
        segments and a `ref_seconds` reference:
          * GPT context: gvc_gpt_warmup for every context class the generation calls of a segment reach (the one-launch steps' buffers,
            weight pack and topology probe; the captured step graphs) -- after it no GPT data-path call allocates or synchronises;
          * ContentVec / DVAE / HiFi-GAN / mel + Perceiver: one pass over zeros of the real shapes (their per-shape graphs and plans).
        num_beams = K > 1: also the beam step graphs of `streams` items x K beams (GPT.generate(num_beams=K, do_sample=False)).
        num_beam_groups = G > 1 (with num_beams = K): the group beam step graphs instead (GPT.generate(num_beams=K, num_beam_groups=G,
        diversity_penalty=..., do_sample=False)).
        contrastive_top_k = K > 1: also the contrastive-search buffers and step graphs of `streams` items x K candidates
        (GPT.generate(top_k=K, do_sample=False, penalty_alpha=a)).
        num_return_sequences = N > 1: also the step graphs of the streams * N rows an N-candidate call decodes
        (GPT.generate(do_sample=True, num_return_sequences=N); the KV fan-out and the candidates' score need no warm-up).
        guidance=True: also the guided step graphs of `streams` items x 2 KV slots (GPT.generate(guidance_scale=s,
        negative_cond_latents=...)), for a negative prompt as long as the conditional one.
        ras_window = K [, ras_threshold]: the calls will use repetition-aware sampling, which runs the full sampling kernel whatever
        top_k is: with top_k == 1 the sampling step graphs of the same shapes are captured as well (with any other top_k they are the
        ones already warmed), so a RAS call neither allocates nor captures.
        presence_penalty / frequency_penalty / penalty_window: the calls will carry these penalties.  Both sampler kernels apply them
        and the table travels in the device-resident call state, so the graphs warmed above are the ones such calls replay: the
        values are validated (ValueError) and nothing more is captured.
        watermarking_config: the calls will carry this green-list watermark (GPT.generate).  It is validated, its table is built on
        the host and uploaded into a slot of the engine's arena (allocated here); both sampler kernels apply it from the
        device-resident call state, so such calls replay the graphs warmed above and neither allocate, upload nor capture.
        No token is generated and no KV slot is left occupied."""
        dev = self.device
        g = self.gpt
        g._need_engine()
        eng = g.engine
        n_src = int(seg_len * self.content_sample_rate)
        wav = torch.zeros(streams, n_src, device=dev)
        wav[:, ::7] = 0.01                                   # (not digital silence: the `wav == 0` frame mask must not swallow the input)
        feat = self.content_extractor.extract_content_features(wav)
        codes = self.content_dvae.get_codebook_indices(feat.transpose(1, 2))
        ref = torch.zeros(1, int(ref_seconds * self.config.audio.sample_rate), device=dev)
        ref[:, ::5] = 0.01
        cond = self.get_gpt_cond_latents(ref, self.config.audio.sample_rate)
        n0 = cond.shape[1] + codes.shape[1] + 3
        top_k = self.config.top_k if top_k is None else top_k
        max_new = int(max_new_tokens or g.max_gen_mel_tokens)
        grp = max(stream_chunk_size, 1)
        # the calls get_generator / _advance will make reach max_keys = n0 + grp ... n0 + max_new: the library warms every context class in
        # that range (its thresholds are its own: gvc_gpt_warmup_range)
        hi = min(n0 + max_new, eng.dims["max_seq"] - 1)
        from genvc_amd.engine import penalty_settings, ras_counts, watermark_settings
        wm = watermark_settings(dict(watermarking_config=watermarking_config), g.num_audio_tokens)
        if wm is not None:
            eng.watermark_entry(wm, hold=False)          # (the slot keeps the table until eight other tables have come after it)
        penalty_settings(dict(presence_penalty=presence_penalty, frequency_penalty=frequency_penalty, penalty_window=penalty_window))
        ras = ras_counts(dict(ras_window=ras_window, ras_threshold=ras_threshold)) is not None
        for k in [top_k] + ([0] if ras and top_k == 1 else []):          # (0: the graphs around the full sampling kernel)
            eng.warmup_range(streams, min(n0 + grp, hi), hi, k)
            if int(num_return_sequences) > 1:
                eng.warmup_range(streams * int(num_return_sequences), min(n0 + grp, hi), hi, k)
        if int(num_beams) > 1 and int(num_beam_groups) > 1:
            eng.warmup_group_beam(streams, int(num_beams), int(num_beam_groups), hi)
        elif int(num_beams) > 1:
            eng.warmup_beam(streams, int(num_beams), hi)
        if contrastive_top_k is not None and int(contrastive_top_k) > 1:
            eng.warmup_contrastive(streams, int(contrastive_top_k), hi)
        if guidance:
            eng.warmup_cfg(streams, hi, top_k)
            if ras and top_k == 1:
                eng.warmup_cfg(streams, hi, 0)
        if self.hifigan is not None:
            lat = torch.zeros(streams, grp, g.model_dim, device=dev)
            for n in {grp, max(1, max_new % grp)}:
                self.hifigan.forward_latents(lat[:, :n].contiguous(), int(self.hifigan_scale_factor))
        torch.cuda.synchronize()
        return self

    @torch.no_grad()
    def inference(self, src_audio, cond_latent, do_sample=True, top_p=0.85, top_k=15, temperature=0.75, num_beams=1,
                  length_penalty=1.0, repetition_penalty=10.0, output_attentions=False, repass_latents=False, generate_kwargs=None,
                  num_return_sequences=None, num_beam_groups=None, diversity_penalty=None, guidance_scale=None, negative_ref_audio=None,
                  return_alignment=False):
        """reference trainers/hifigan_trainer.py:457-500: one source segment [1,T] + conditioning latents -> waveform
        [1,1,1024 n]: ContentVec -> content codes -> generate -> strip stop tokens -> latent re-pass -> x4 linear
        interpolation -> HiFi-GAN.  (The reference's 0-d collapse at exactly one non-stop token, SURVEY appendix B.9, is
        guarded: boolean indexing keeps the dimension.)  The latents are the decode loop's own unless `repass_latents=True`
        (inference_utils._segment_latents).  generate_kwargs (extension): more GPT.generate kwargs (the logits processors:
        min_new_tokens, no_repeat_ngram_size, ...; typical_p, epsilon_cutoff, eta_cutoff; ras_window; presence_penalty,
        frequency_penalty, penalty_window), merged over the ones above.
        num_return_sequences = N > 1 (the keyword, or in generate_kwargs; sampling only): a LIST of N waveforms, the candidates of
        GPT.generate(num_return_sequences=N) in row order, each stripped of its stop tokens and vocoded from the decode loop's own
        latents (or the re-pass with `repass_latents=True`); `last_sequence_logprobs` / `last_sequence_lengths` hold their scores
        (GPT.sequence_logprobs: the raw model distribution).  N = 1 returns the one waveform, not a list.
        num_beam_groups = G > 1 with diversity_penalty > 0 (and num_beams = K, do_sample=False): group (diverse) beam search; with
        num_return_sequences = N <= K the N waveforms are its N best hypotheses, `last_beam_scores` their scores.
        guidance_scale = s != 1 (the keyword, or in generate_kwargs): classifier-free guidance; the negative prompt's conditioning
        latents are generate_kwargs["negative_cond_latents"] when given (synthesize_utt_chunked computes them once per utterance),
        else those of negative_ref_audio = (wav, sample rate), default this source segment.
        return_alignment=True: (waveform, alignment) -- alignment fp32 [n_codes, Tc], the attention of each generated acoustic code over
        the Tc content codes of the segment (GPT.trace: the head / layer mean, one more teacher-forced pass; a row sums to at most 1).
        Not with num_return_sequences > 1."""
        feat = self.content_extractor.extract_content_features(src_audio)
        codes = self.content_dvae.get_codebook_indices(feat.transpose(1, 2))
        kw = dict(do_sample=do_sample, top_p=top_p, top_k=top_k, temperature=temperature, num_beams=num_beams,
                  length_penalty=length_penalty, repetition_penalty=repetition_penalty, output_attentions=output_attentions)
        kw.update(generate_kwargs or {})
        if num_return_sequences is not None:
            kw["num_return_sequences"] = num_return_sequences
        if num_beam_groups is not None:
            kw["num_beam_groups"] = num_beam_groups
        if diversity_penalty is not None:
            kw["diversity_penalty"] = diversity_penalty
        from genvc_amd.inference.inference_utils import _guided_kwargs
        kw = _guided_kwargs(self, kw, guidance_scale, negative_ref_audio, src_audio)
        from genvc_amd.layers.gpt import _num_return
        if _num_return(kw) > 1:
            if return_alignment:
                raise NotImplementedError("return_alignment=True with num_return_sequences > 1 is not implemented: GPT.trace serves each "
                                          "candidate's codes")
            return self._inference_candidates(cond_latent, codes, kw, repass_latents)
        gen = self.gpt.generate(cond_latent, codes, **kw)
        gen = getattr(gen, "sequences", gen)[0]
        gen = gen[gen != self.gpt.stop_audio_token]
        if gen.numel() == 0:
            wav = torch.zeros(1, 1, 0, device=self.device)
            return (wav, torch.zeros(0, codes.shape[-1], device=self.device)) if return_alignment else wav
        wav = self._vocode_segment(cond_latent, codes, gen, repass_latents)
        if return_alignment:
            return wav, self.gpt.trace(cond_latent, codes, gen.unsqueeze(0), output_attentions=False).alignment[0]
        return wav

    def _vocode_segment(self, cond_latent, codes, gen, repass_latents, row=0):
        """the stop-free tokens `gen` of row `row` of the last generate call -> waveform [1, 1, 1024 n] (latents, x4 linear
        interpolation, HiFi-GAN: trainers/hifigan_trainer.py:489-500)"""
        from genvc_amd.inference.inference_utils import _segment_latents
        lat = _segment_latents(self, cond_latent, codes, gen, repass_latents, row=row)
        mel_input = torch.nn.functional.interpolate(lat.transpose(1, 2), scale_factor=[self.hifigan_scale_factor],
                                                    mode="linear").squeeze(1)
        return self.hifigan.forward(mel_input)

    def _inference_candidates(self, cond_latent, codes, kw, repass_latents):
        """inference() for num_return_sequences = N > 1: one generate call, then each candidate row vocoded on its own"""
        g = self.gpt
        rows = g.generate(cond_latent, codes, **kw)
        sampled = g.last_latents is not None
        self.last_sequence_logprobs = g.last_sequence_logprobs if sampled else None
        self.last_sequence_lengths = g.last_sequence_lengths if sampled else None
        self.last_beam_scores = None if sampled else g.last_beam_scores
        out = []
        for j in range(rows.shape[0]):
            gen = rows[j][rows[j] != g.stop_audio_token]
            if gen.numel() == 0:
                out.append(torch.zeros(1, 1, 0, device=self.device))
            else:
                out.append(self._vocode_segment(cond_latent, codes, gen, repass_latents, row=j))
        return out


def content_pad_samples(text_frame_rate, content_sample_rate):
    """zero samples appended to the content waveform (gpt_trainer.py:240)"""
    return int(text_frame_rate * content_sample_rate)


def default_text_lengths(wav_lengths, sample_rate, text_frame_rate=0.02):
    """dataset.py:56,154: wav_lengths // (int(text_frame_rate * sample_rate) * 4)"""
    return torch.as_tensor(wav_lengths).to(torch.long) // (int(text_frame_rate * sample_rate) * 4)


class _CondFuture:
    def __init__(self, model, audio, sr, length, chunk_length, after=None):
        if not audio.is_cuda:
            audio = audio.to(model.device)
        main = torch.cuda.current_stream(audio.device)
        side = getattr(model, "_cond_stream", None)
        if side is None:
            side = model._cond_stream = torch.cuda.Stream(device=audio.device)
        if after is not None:
            side.wait_event(after)                   # the audio is ready at `after`; what the caller enqueued behind it runs beside this chain
        else:
            side.wait_stream(main)                   # (the audio may still be in flight on the caller's stream)
        audio.record_stream(side)
        with torch.cuda.stream(side):
            self.cond = model.get_gpt_cond_latents(audio, sr, length, chunk_length)
        self.side = side
        # residency before issue: a GPT call on another stream (a one-launch step needs every CU) waits for this chain first
        done = torch.cuda.Event()
        done.record(side)
        eng = getattr(model.gpt, "engine", None)
        if eng is not None:
            eng.watch_stream(done)

    def result(self):
        main = torch.cuda.current_stream(self.cond.device)
        main.wait_stream(self.side)
        self.cond.record_stream(main)
        return self.cond


def build_model(config, device, content_extractor=None, hifigan=None, max_slots=8, weight_dtype="fp32"):
    model = GenVCModel(config, content_extractor, hifigan)
    return model, (lambda: _finish(model, device, max_slots, weight_dtype))


def _finish(model, device, max_slots, weight_dtype="fp32"):
    model.eval()
    model.to(device)
    # prefill capacity: every slot may bring a 6 s segment (110 rows) into one batched call
    model.gpt.init_gpt_for_inference(max_slots=max_slots, max_rows=max(4096, 128 * max_slots), weight_dtype=weight_dtype)
    mb = max(2, max_slots)
    model.content_dvae.bind(max_batch=max(8, max_slots))
    if hasattr(model.content_extractor, "bind"):
        if hasattr(model.content_extractor, "max_batch"):
            model.content_extractor.max_batch = mb
        model.content_extractor.bind()
    if model.hifigan is not None:
        model.hifigan.bind(max_batch=mb)
    return model


@torch.inference_mode()
def model_init(checkpoint_path, device, content_extractor=None, hifigan=None, weight_dtype="fp32"):
    ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
    config = gcfg.default_config()
    _merge(config, ckpt["config"])
    model, finish = build_model(config, device, content_extractor, hifigan, weight_dtype=weight_dtype)
    model.missing_checkpoint_keys, _ = _load_checked(model, ckpt["model"])    # model_init.py:22 (strict=False)
    finish()
    print("Model initialized")
    return model, config


@torch.inference_mode()
def model_init_synthetic(config=None, seed=1, device="cuda", max_slots=8, weight_dtype="fp32", with_acoustic=False):
    """No checkpoint ships with the reference: deterministic synthetic weights of the same architecture.  with_acoustic=True (or a
    config with `acoustic_dvae_config`): also the acoustic DVAE, its codebook at standard deviation 0.05 (at 1.0 the synthetic encoder
    output lies far inside the codebook and a handful of codes is ever chosen)."""
    from .. import synth
    config = config or gcfg.default_config(with_acoustic=with_acoustic)
    if with_acoustic and config.get("acoustic_dvae_config") is None:
        config["acoustic_dvae_config"] = gcfg.to_attr(dict(gcfg.DEFAULT_ACOUSTIC_DVAE))
    model, finish = build_model(config, device, max_slots=max_slots, weight_dtype=weight_dtype)
    dims = gcfg.gpt_dims(config.model_args)
    w = {"gpt." + k: v for k, v in synth.make_weights(seed, synth.gpt_weight_spec(dims), device=device).items()}
    w.update({"content_dvae." + k: v for k, v in
              synth.make_weights(seed, synth.dvae_weight_spec(config.content_dvae_config), device=device).items()})
    if model.acoustic_dvae is not None:
        w.update({"acoustic_dvae." + k: v for k, v in
                  synth.make_weights(seed, synth.dvae_full_weight_spec(config.acoustic_dvae_config, codebook_scale=0.05),
                                     device=device).items()})
    if model.hifigan is not None:
        w.update({"hifigan." + k: v for k, v in
                  synth.make_weights(seed, synth.hifigan_weight_spec(config.vocoder_config), device=device).items()})
    if isinstance(model.content_extractor, ContentvecExtractor):
        w.update({"content_extractor.model." + k: v for k, v in
                  synth.make_weights(seed, synth.hubert_weight_spec(model.content_extractor.cfg), device=device).items()})
    model.to(device)
    missing, unexpected = model.load_state_dict(w, strict=False)
    assert not unexpected, unexpected
    finish()
    return model, config


@torch.inference_mode()
def synthetic_assistant(config, layers, seed=2, device="cuda", max_slots=8, weight_dtype="fp32"):
    """A draft GPT for GPT.generate(assistant_model=...): the architecture of config.model_args with `layers` layers, deterministic
    synthetic weights of its own (a demonstration of the mode: such a draft agrees with the target about as often as chance)."""
    from .. import synth
    from ..layers.gpt import GPT
    a = gcfg.to_attr(dict(config.model_args, gpt_layers=int(layers)))
    g = GPT(layers=a.gpt_layers, model_dim=a.gpt_n_model_channels, heads=a.gpt_n_heads,
            max_text_tokens=a.gpt_max_text_tokens, max_mel_tokens=a.gpt_max_audio_tokens,
            max_prompt_tokens=a.gpt_max_prompt_tokens, number_text_tokens=a.gpt_number_text_tokens,
            start_text_token=a.gpt_start_text_token, stop_text_token=a.gpt_stop_text_token,
            num_audio_tokens=a.gpt_num_audio_tokens, start_audio_token=a.gpt_start_audio_token,
            stop_audio_token=a.gpt_stop_audio_token, code_stride_len=a.gpt_code_stride_len)
    g.load_state_dict(synth.make_weights(seed, synth.gpt_weight_spec(gcfg.gpt_dims(a)), device=device), strict=False)
    g.eval()
    g.to(device)
    return g.init_gpt_for_inference(max_slots=max_slots, weight_dtype=weight_dtype)


_REQUIRED_PREFIXES = ("gpt.", "content_dvae.", "hifigan.", "content_extractor.model.")


def _load_checked(model, state):
    """load_state_dict(strict=False) as the reference does (model_init.py:22: the checkpoint also holds discriminators, the
    acoustic DVAE ...), but a checkpoint that LACKS a tensor of the inference path would leave a placeholder (zeros / random)
    in the engines and produce garbage audio silently: those keys are reported.  Weight-norm tensors saved by newer torch
    (`parametrizations.weight.original0/1`) are renamed to the `weight_g` / `weight_v` the reference's checkpoints carry."""
    state = dict(state)
    for k in list(state):
        if ".parametrizations.weight.original" in k:
            new = k.replace(".parametrizations.weight.original0", ".weight_g").replace(".parametrizations.weight.original1", ".weight_v")
            state[new] = state.pop(k)
    missing, unexpected = model.load_state_dict(state, strict=False)
    lost = [k for k in missing if k.startswith(_REQUIRED_PREFIXES)
            and not k.endswith((".attn.bias", ".attn.masked_bias"))]
    if lost:
        raise RuntimeError(f"checkpoint lacks {len(lost)} tensors of the inference path, e.g. {lost[:6]} "
                           f"(unexpected keys: {len(unexpected)})")
    return missing, unexpected


def _merge(dst, src):
    for k, v in dict(src).items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = gcfg.to_attr(v)
