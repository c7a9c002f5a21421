"""`IndexTTS2` of IndexTTS-2 (`indextts/infer_v2.py`, BASELINE.json configs[3]) with the reference's constructor / `infer()`
signatures and the hot stages on the HIP engine.

Differences from the v2.5 pipeline (`indextts_amd/infer_v2_5.py`, whose batching, caching and output handling are inherited):
  * `self.gpt` is `UnifiedVoice` in the reference's default conditioning mode (34 conditioning tokens: 32 Conformer + Perceiver
    speaker latents + emo_vec, two speed embeddings; infer_v2.py:98, model_v2.py:767-773); the speaker / emotion encoders are
    prompt-side PyTorch modules reached through `gpt.conditioning_fn` and the frontend;
  * after decoding, the teacher-forced latent pass `self.gpt(...)` (infer_v2.py:636-651) runs on the engine
    (`itts_gpt_forward_latent`) and its output goes through `s2mel.models['gpt_layer']`;
  * the content features are `semantic_codec.quantizer.vq2emb(codes) + latent` (no Vocos decode), the mel length is
    `(code_lens * 1.72).long()` (:659-662);
  * the speaker prompt's content condition goes through the codec's `quantize` half first (`prompt_condition`, :465-479).
"""
import time
import warnings
from typing import List

import torch

from .infer_v2_5 import PCM16_MAX, Frontend, IndexTTS2 as _IndexTTS2V25  # noqa: F401


class ChunkLatents:
    """The latents that go with every chunk `UnifiedVoice.generate_chunks` yields, from a `LatentSession`.  Chunk k covers the codes
    [k * stride, k * stride + width): the first chunk is all new; a later chunk starts with codes the session has already seen (its
    `overlap_size` head), whose latents are the tail kept from the chunk before, and only the rest is appended.  `chunks` records, per
    chunk, `dict(pos, new_from, codes, latent, lens)`: the latents of columns `new_from:` are the ones this chunk added."""

    def __init__(self, session, chunk_size: int, overlap_size: int):
        self.session, self.stride, self.overlap = session, int(chunk_size) - int(overlap_size), int(overlap_size)
        self.k, self.appended, self.tail, self.chunks = 0, 0, None, []

    def __call__(self, codes: torch.Tensor, code_lens=None) -> torch.Tensor:
        pos, width = self.k * self.stride, int(codes.shape[1])
        head = self.appended - pos                                   # columns of this chunk the session has already seen
        if head < 0 or (self.k > 0 and head > self.overlap):
            raise RuntimeError(f"ChunkLatents: chunk {self.k} starts at code {pos} but {self.appended} codes have been appended")
        new = self.session.append(codes[:, head:]) if width > head else None
        parts = ([self.tail[:, self.tail.shape[1] - head:]] if head > 0 else []) + ([new] if new is not None else [])
        latent = torch.cat(parts, dim=1)[:, :width]
        if new is not None:
            self.appended += int(new.shape[1])
            keep = new if self.tail is None else torch.cat([self.tail, new], dim=1)
            self.tail = keep[:, max(0, keep.shape[1] - self.overlap):] if self.overlap > 0 else keep[:, :0]
        self.chunks.append(dict(pos=pos, new_from=min(head, width), codes=codes, latent=latent, lens=code_lens))
        self.k += 1
        return latent


class IndexTTS2(_IndexTTS2V25):
    USE_GPT_LATENT = True
    SPK_COND_MODE = "conformer"            # infer_v2.py:98: `UnifiedVoice(**cfg.gpt)`, the default conditioning mode (no spk_emb_proj.*)

    @staticmethod
    def _bigvgan_dir(model_dir, aux_paths=None):
        """infer_v2.py:176-177: `aux_paths["bigvgan"]`; `ensure_models_available(model_dir)` (utils/model_download.py:213-214) places it
        at `<model_dir>/hf_cache/bigvgan`, which is where it is looked for when no `aux_paths` is given (no downloads here)."""
        import os
        if aux_paths and "bigvgan" in aux_paths:
            return aux_paths["bigvgan"]
        return os.path.join(model_dir, "hf_cache", "bigvgan")

    def __init__(self, cfg_path="checkpoints/config.yaml", model_dir="checkpoints", use_fp16=False, device=None, use_cuda_kernel=None,
                 use_deepspeed=False, use_accel=False, use_torch_compile=False, use_qwen_emo=True, aux_paths=None, *, frontend=None,
                 gpt=None, bigvgan=None, cfg=None, semantic_codec=None, s2mel=None, codes_to_mel="auto"):
        """infer_v2.py:37-41.  `use_fp16` selects the engine's reduced-precision (bf16) GPT mode; QwenEmotion (text -> emotion
        vector) is a prompt-side LLM: when no frontend providing it is injected, `use_emo_text` raises like the reference does
        without the model."""
        super().__init__(cfg_path=cfg_path, model_dir=model_dir, use_bf16=use_fp16, device=device, use_cuda_kernel=use_cuda_kernel,
                         use_deepspeed=use_deepspeed, use_accel=use_accel, use_torch_compile=use_torch_compile, use_qwen_emo=False,
                         frontend=frontend, gpt=gpt, bigvgan=bigvgan, cfg=cfg, semantic_codec=semantic_codec, s2mel=s2mel,
                         aux_paths=aux_paths, codes_to_mel=codes_to_mel)
        self.use_fp16 = bool(use_fp16)
        self.aux_paths = aux_paths
        self.model_version = (cfg or self.cfg).get("version", 2.0)

    # ---- API: the reference v2 signatures (infer_v2.py:371-400) -- no `lang`, `duration_factor`, `text_normalization` -------------
    def infer(self, spk_audio_prompt, text, output_path, emo_audio_prompt=None, emo_alpha=1.0, emo_vector=None, use_emo_text=False,
              emo_text=None, use_random=False, interval_silence=200, verbose=False, max_text_tokens_per_segment=120,
              stream_return=False, more_segment_before=0, **generation_kwargs):
        gen = self.infer_generator(spk_audio_prompt, text, output_path, emo_audio_prompt, emo_alpha, emo_vector, use_emo_text, emo_text,
                                   use_random, interval_silence, verbose, max_text_tokens_per_segment, stream_return,
                                   more_segment_before, **generation_kwargs)
        if stream_return:
            return gen
        try:
            return list(gen)[0]
        except IndexError:
            return None

    def infer_generator(self, spk_audio_prompt, text, output_path, emo_audio_prompt=None, emo_alpha=1.0, emo_vector=None,
                        use_emo_text=False, emo_text=None, use_random=False, interval_silence=200, verbose=False,
                        max_text_tokens_per_segment=120, stream_return=False, quick_streaming_tokens=0, **generation_kwargs):
        yield from self._infer_impl(spk_audio_prompt, text, output_path, None, emo_audio_prompt, emo_alpha, emo_vector, use_emo_text,
                                    emo_text, use_random, interval_silence, verbose, max_text_tokens_per_segment, stream_return, 1.0,
                                    True, generation_kwargs)

    @staticmethod
    def _segment_text(segment_tokens: List[torch.Tensor]):
        """(text (B, L) int32 right-padded with the stop text id, text_lens (B,)) of a batch of segments.  The teacher-forced pass sees
        `[start, ids, stop]` (infer_v2.py:558-560,639-642: the v2 reference tokenises a segment WITHOUT a trailing stop id and `forward`
        pads one on).  The Frontend protocol appends stop id 1 to every segment (the v2.5 convention, infer_v2_5.py:726); it is not part
        of the text, so the length handed to the latent pass excludes trailing stop ids."""
        B = len(segment_tokens)
        L = max(int(t.numel()) for t in segment_tokens)
        text = torch.full((B, L), 1, dtype=torch.int32)                 # stop_text_token right padding
        text_lens = []
        for i, t in enumerate(segment_tokens):
            flat = t.reshape(-1).to(torch.int32)
            text[i, : flat.numel()] = flat
            n = int(flat.numel())
            if n > 0 and int(flat[n - 1]) == 1:          # exactly the ONE stop id the Frontend protocol appends (ids inside a segment are >= 2)
                n -= 1
            if n <= 0:
                raise ValueError(f"segment {i} holds no text tokens (the reference never synthesises an empty segment, infer_v2.py:566-567)")
            text_lens.append(n)
        return text, torch.tensor(text_lens)

    def infer_stream(self, spk_audio_prompt, texts, emo_audio_prompt=None, emo_alpha=1.0, chunk_size: int = 100, overlap_size: int = 20,
                     max_text_tokens_per_segment=120, **generation_kwargs):
        """Streaming synthesis of a batch of single-segment texts with IndexTTS-2 (the reference's streaming pipeline,
        backends/trt/pipeline/streaming.py:57-198, pipeline.py:459-554: every chunk of codes goes to codes -> audio together with that
        chunk's LATENT).  Same yield protocol as the v2.5 `infer_stream`: `(22050, [int16 array | None per text], [done per text])` per GPT
        chunk; `num_beams` is forced to 1.  The chunk's latents come from a KV-cached teacher-forced session (`UnifiedVoice.latent_session`)
        that runs beside the suspended decode loop: per chunk only the NEW codes are appended (the first chunk whole, later ones without
        their `overlap_size` head, whose latents are kept from the chunk before), so the latents are those `infer()` computes on the
        finished utterance, at O(chunk) cost per chunk.  Rows that have finished are fed their stop-token padding.
        `cfm_noise="request"`: the flow-matching noise of chunk k of row i is keyed by (`seed`, i, chunk = k), as in the v2.5 `infer_stream`."""
        from .streaming import StreamingDecoder
        from .gpt import refuse_code_prefix
        gk = dict(generation_kwargs)
        refuse_code_prefix(gk, "infer_stream (IndexTTS-2)")
        from .output import refuse_audio_format
        refuse_audio_format(gk, "infer_stream (IndexTTS-2)")
        keyed = self._cfm_noise_mode(gk) == "request"
        if keyed:
            self._need_engine_s2mel("cfm_noise='request'")
            if gk.get("seed") is None:
                gk["seed"] = self.gpt._seed(None, True, None)
        if int(overlap_size) >= int(chunk_size):
            raise ValueError(f"overlap_size ({overlap_size}) must be less than chunk_size ({chunk_size})")
        if emo_audio_prompt is None:
            emo_audio_prompt, emo_alpha = spk_audio_prompt, 1.0
        bundle = dict(self._speaker(spk_audio_prompt))
        emovec = self._emovec(bundle, emo_audio_prompt, emo_alpha, None, False)
        seg_tokens = []
        for text in texts:
            segs = self.frontend.text_segments(text, None, max_text_tokens_per_segment, True, self.gpt.n_text_pos)
            if len(segs) != 1:
                raise ValueError("infer_stream takes texts of one segment each (split long texts with the frontend first)")
            seg_tokens.append(segs[0])
        gk.pop("do_sample", None)
        gk.pop("num_beams", None)
        max_mel_tokens = gk.pop("max_mel_tokens", 1500)
        gen = dict(do_sample=True, top_p=gk.pop("top_p", 0.8), top_k=gk.pop("top_k", 30), temperature=gk.pop("temperature", 0.8),
                   repetition_penalty=gk.pop("repetition_penalty", 10.0), length_penalty=gk.pop("length_penalty", 0.0), num_beams=1, **gk)
        dev = self.device
        B = len(seg_tokens)
        text, text_lens = self._segment_text(seg_tokens)
        spk_cond_emb = bundle["spk_cond_emb"]
        n_spk = min(int(spk_cond_emb.shape[-1]), int(spk_cond_emb.shape[1]))
        lat1 = self.gpt.get_conditioning(spk_cond_emb.transpose(1, 2), torch.tensor([n_spk], device=spk_cond_emb.device))
        conds = self.gpt.conds_latent_v2(lat1.expand(B, -1, -1), emovec)
        inputs_embeds, attention_mask, max_new, hf = self.gpt.inference_speech_stream(
            spk_cond_emb, text.to(dev), chunk_size, overlap_size, emo_vec=emovec, conds_latent=conds, max_generate_length=max_mel_tokens, **gen)
        emo_b = emovec.expand(B, -1) if emovec.shape[0] == 1 else emovec
        session = self.gpt.latent_session(self.gpt.latent_conds(lat1.expand(B, -1, -1), emo_b, torch.zeros(B, dtype=torch.long)),
                                          text.to(dev), text_lens, max_codes=max_new, max_append=min(int(chunk_size), max_new))
        track = ChunkLatents(session, chunk_size, overlap_size)
        self.last_stream_latents = track.chunks
        up = self.bigvgan.total_up

        def codes_to_audio(codes, code_lens):
            latent = track(codes, code_lens)                            # the chunk's latents travel inside this closure
            lens = torch.as_tensor(code_lens).to(torch.int32).cpu().clamp(min=1)      # finished rows render one frame, dropped by the decoder
            n = codes.shape[0]
            s2kw = dict(noise_keys=([int(gen["seed"])] * n, list(range(n)), [dec.chunk_index] * n)) if keyed else {}      # (seed, row, chunk)
            mel, mel_lens = self.codes_latent_to_mel(codes, lens, latent, bundle, **s2kw)
            wav = self.bigvgan(mel.float(), lens=mel_lens)
            return [wav[i, 0, : int(mel_lens[i]) * up].float().cpu().numpy() for i in range(wav.shape[0])]

        dec = StreamingDecoder(self.gpt, codes_to_audio, chunk_size=chunk_size, overlap_size=overlap_size)     # 1.72 frames per code
        self.last_stream = dec
        try:
            yield from dec.generate(inputs_embeds, attention_mask, max_new, **hf)
        finally:
            session.close()

    def _synthesize(self, segment_tokens: List[torch.Tensor], lang_ids, bundle, emovec, duration_factor, generation_kwargs,
                    max_text_tokens_per_segment) -> List[torch.Tensor]:
        gk = dict(generation_kwargs)
        from .gpt import refuse_code_prefix
        refuse_code_prefix(gk, "IndexTTS-2 (v2)")
        gk.pop("do_sample", None)                       # popped and ignored by the reference (infer_v2.py:537,590)
        top_p, top_k = gk.pop("top_p", 0.8), gk.pop("top_k", 30)
        temperature = gk.pop("temperature", 0.8)
        length_penalty = gk.pop("length_penalty", 0.0)
        num_beams = gk.pop("num_beams", 3)
        repetition_penalty = gk.pop("repetition_penalty", 10.0)
        max_mel_tokens = gk.pop("max_mel_tokens", 1500)
        dev = self.device
        B = len(segment_tokens)
        s2kw = {}
        if self._cfm_noise_mode(gk) == "request":          # (popped here: it never reaches inference_speech) noise of row i keyed by (seed, i)
            self._need_engine_s2mel("cfm_noise='request'")
            if gk.get("seed") is None:
                gk["seed"] = self.gpt._seed(None, True, None)
            s2kw["noise_keys"] = ([int(gk["seed"])] * B, list(range(B)))
        text, text_lens = self._segment_text(segment_tokens)
        spk_cond_emb, emo_cond_emb = bundle["spk_cond_emb"], bundle.get("emo_cond_emb", bundle["spk_cond_emb"])
        t0 = time.perf_counter()
        # one batch of B segments: the speaker latents are the same for every row (one speaker prompt).  The reference hands the
        # feature WIDTH over as the length (infer_v2.py:646, model_v2.py:761): "every frame valid" for prompts under 1024 frames
        n_spk = min(int(spk_cond_emb.shape[-1]), int(spk_cond_emb.shape[1]))
        lat1 = self.gpt.get_conditioning(spk_cond_emb.transpose(1, 2), torch.tensor([n_spk], device=spk_cond_emb.device))
        conds = self.gpt.conds_latent_v2(lat1.expand(B, -1, -1), emovec)
        codes, speech_conditioning_latent = self.gpt.inference_speech(
            spk_cond_emb, text.to(dev), emo_cond_emb, emo_vec=emovec, conds_latent=conds, do_sample=True, top_p=top_p, top_k=top_k,
            temperature=temperature, num_return_sequences=1, length_penalty=length_penalty, num_beams=num_beams,
            repetition_penalty=repetition_penalty, max_generate_length=max_mel_tokens, **gk)
        torch.cuda.synchronize() if torch.cuda.is_available() else None
        t1 = time.perf_counter()
        if codes.shape[1] > 0 and (codes[:, -1] != self.stop_mel_token).any():
            warnings.warn(f"WARN: generation stopped due to exceeding `max_mel_tokens` ({max_mel_tokens}). "
                          f"Consider reducing `max_text_tokens_per_segment`({max_text_tokens_per_segment}) or increasing "
                          f"`max_mel_tokens`.", category=RuntimeWarning)
        codes, code_lens = self.trim_codes(codes)
        # teacher-forced latent pass (infer_v2.py:636-651) on the trimmed codes.  The reference runs it per segment at batch 1; the pass
        # has no attention mask (get_logits, model_v2.py:534), so a row padded to a longer neighbour's text / code length would see the
        # padding: rows are grouped by (text length, code length) and every group runs unpadded -- each row gets exactly its batch-1 result
        emo_b = emovec.expand(B, -1) if emovec.shape[0] == 1 else emovec
        cl = [int(v) for v in code_lens]
        groups = {}
        for b in range(B):
            groups.setdefault((int(text_lens[b]), cl[b]), []).append(b)
        latent = None
        for (tl, ml), rows in groups.items():
            if ml == 0:
                continue
            idx = torch.tensor(rows, device=codes.device)
            n = len(rows)
            lat_g = self.gpt(lat1.expand(n, -1, -1), text[rows][:, :tl].to(dev), torch.full((n,), tl), codes[idx][:, :ml],
                             torch.full((n,), ml), emo_cond_emb, cond_mel_lengths=None, emo_cond_mel_lengths=None, emo_vec=emo_b[rows],
                             use_speed=torch.zeros(n, dtype=torch.long))
            if latent is None:
                latent = torch.zeros(B, codes.shape[1], lat_g.shape[-1], dtype=torch.float32, device=codes.device)
            latent[idx, :ml] = lat_g.to(latent.device, torch.float32)
        if latent is None:                                     # every row stopped at once: nothing to render
            latent = torch.zeros(B, codes.shape[1], 1, dtype=torch.float32, device=codes.device)
        torch.cuda.synchronize() if torch.cuda.is_available() else None
        t2 = time.perf_counter()
        mel, mel_lens = self.codes_latent_to_mel(codes, code_lens, latent, bundle, **s2kw)
        torch.cuda.synchronize() if torch.cuda.is_available() else None
        t3 = time.perf_counter()
        wav = self.bigvgan(mel.float(), lens=mel_lens)
        wav = torch.clamp(PCM16_MAX * wav, -PCM16_MAX, PCM16_MAX)
        up = self.bigvgan.total_up
        out = [wav[i, :, : int(mel_lens[i]) * up].cpu() for i in range(wav.shape[0])]
        t4 = time.perf_counter()
        self.last_timing = dict(gpt=t1 - t0, gpt_forward=t2 - t1, s2mel=t3 - t2, bigvgan=t4 - t3)
        return out

    @torch.no_grad()
    def prompt_condition(self, spk_cond_emb: torch.Tensor, ref_mel_frames: int) -> torch.Tensor:
        """The speaker prompt's content condition of IndexTTS-2 (infer_v2.py:465-479) on the engine: `_, S_ref = semantic_codec.quantize(
        spk_cond_emb)` (down conv, Vocos encoder, FVQ search + out_project) -> `length_regulator(S_ref, ylens=[ref_mel.size(2)])`.
        spk_cond_emb (1, T, 1024) w2v-bert features -> (1, ref_mel_frames, 512).  (v2.5 regulates spk_cond_emb directly, infer_v2_5.py:651-656.)"""
        if self.s2mel is None or self.semantic_codec is None:
            raise RuntimeError("prompt_condition needs the engine's semantic codec and s2mel stages")
        _, S_ref = self.semantic_codec.quantize(spk_cond_emb)
        return self.s2mel.models["length_regulator"](S_ref, ylens=torch.tensor([int(ref_mel_frames)]), n_quantizers=3, f0=None)[0]

    def codes_latent_to_mel(self, codes, code_lens, latent, bundle, diffusion_steps=25, inference_cfg_rate=0.7, noise=None, noise_keys=None,
                            noise_temperature=1.0):
        """infer_v2.py:653-676 for a batch of segments: gpt_layer(latent) + vq2emb(codes) -> length_regulator ->
        [prompt_condition | cond] -> cfm.inference -> drop the prompt frames, each row at its own lengths.  `noise_keys`, `noise_temperature` and
        per-row `diffusion_steps` / `inference_cfg_rate` as in `s2mel.codes_to_mel`."""
        if self.s2mel is None or self.semantic_codec is None:
            if noise_keys is not None:
                self._need_engine_s2mel("noise_keys")
            return self.frontend.codes_latent_to_mel(codes, code_lens, latent, bundle)
        from .s2mel import cfm_inference_rows
        lens = [int(v) for v in code_lens]
        lat = self.s2mel.models["gpt_layer"](latent)                                         # (B, T, 1024)
        S_infer = self.semantic_codec.quantizer.vq2emb(codes.unsqueeze(1)).transpose(1, 2) + lat[:, : codes.shape[1]]
        target = [int(n * 1.72) for n in lens]                                               # (code_lens * 1.72).long()
        reg, cfm = self.s2mel.models["length_regulator"], self.s2mel.models["cfm"]
        cond = reg(S_infer, ylens=torch.tensor(target), n_quantizers=3, f0=None, xlens=lens, frame_lens=target)[0]
        prompt_condition, ref_mel, style = bundle["prompt_condition"], bundle["ref_mel"], bundle["style"]
        Tp, B = int(prompt_condition.shape[1]), codes.shape[0]
        total = [Tp + t for t in target]
        cat = torch.zeros(B, max(total), cond.shape[-1], dtype=torch.float32, device=cond.device)
        cat[:, :Tp] = prompt_condition.to(cond.device, torch.float32)
        for b in range(B):
            cat[b, Tp:total[b]] = cond[b, : target[b]]
        mel = cfm_inference_rows(cfm, cat, total, ref_mel, style, diffusion_steps, inference_cfg_rate, noise=noise, frame_lens=total,
                                 noise_keys=noise_keys, temperature=noise_temperature)
        return mel[:, :, Tp:].contiguous(), torch.tensor(target, dtype=torch.int32)
