"""`IndexTTS2` (v2.5) pipeline class with the reference's constructor / `infer()` / `infer_generator()` signatures,
with the two hot stages re-routed to the HIP engine.

Reference mirrored: `indextts/infer_v2_5.py::IndexTTS2` (`__init__` :77-279, `infer` :506-567, `infer_generator`
:570-899).  What changes behind the API:
  * `self.gpt` is `indextts_amd.gpt.UnifiedVoice` (decode on the HIP engine), `self.bigvgan` is
    `indextts_amd.bigvgan.BigVGAN`;
  * all text segments of one call are decoded as ONE left-padded GPT batch and vocoded as ONE ragged BigVGAN batch
    (the reference loops segment by segment, `:749`); per-segment results are unchanged (padding invariance is a tested
    property), and `infer_batch()` extends the same to many utterances;
  * codes -> mel (semantic-codec decode, length regulator, 25-step CFG flow matching) runs on the HIP engine too when its stages are
    given or buildable from the frontend's state dicts (`codes_to_mel=` "auto" / "engine" / "frontend", recorded in
    `self.codes_to_mel_mode`); "frontend" keeps that stage on the frontend's PyTorch modules;
  * what is NOT on the engine -- audio file decoding, text normalisation + tokenizer + segment splitting, the QwenEmotion LLM -- is
    reached through a `frontend` object.  `ReferenceFrontend` builds the reference's own modules from the reference package +
    checkpoint directory (needs the reference's `indextts` package, torchaudio, librosa, ... -- none exist in the build/bench images,
    so that class is exercised only where they do) and moves the prompt encoders / DSP onto the engine where their configuration
    is the shipped one; `indextts_amd.frontend.EngineFrontend*` need no reference package; tests inject a stub with the same methods.
There is no silent fallback: a missing frontend dependency raises at construction.
"""
import os
import time
import warnings
import wave
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

PCM16_MAX = 32767.0


def save_pcm_wav(path: str, wav: torch.Tensor, sampling_rate: int):
    """16-bit PCM WAV writer for a PCM-scale (+-32767) waveform (C, T) -- `indextts/utils/common.py:38-58` semantics
    (normalise by 32767, clamp to [-1, 1], encode PCM_S16) without the torchaudio dependency."""
    w = (wav.detach().to("cpu", torch.float32) / PCM16_MAX).clamp_(-1.0, 1.0)
    pcm = torch.round(w * PCM16_MAX).to(torch.int16).numpy()
    if pcm.ndim == 1:
        pcm = pcm[None, :]
    with wave.open(path, "wb") as f:
        f.setnchannels(pcm.shape[0])
        f.setsampwidth(2)
        f.setframerate(int(sampling_rate))
        f.writeframes(np.ascontiguousarray(pcm.T).tobytes())


class Frontend:
    """Everything outside the hot path, as the pipeline consumes it.  Shapes follow the reference."""

    def speaker_bundle(self, spk_audio_prompt) -> Dict[str, torch.Tensor]:
        """-> {style (1,192), spk_cond_emb (1,T,1024), ref_mel (1,80,Tm), prompt_condition (1,Tm,512)}  (:620-667)"""
        raise NotImplementedError

    def emo_cond(self, emo_audio_prompt) -> torch.Tensor:            # (:682-697)
        raise NotImplementedError

    def speaker_bundles(self, prompts) -> List[Dict[str, torch.Tensor]]:
        """One bundle per prompt, in order.  The default encodes them one at a time; a front end that can encode N prompts in one pass
        overrides it (`indextts_amd.frontend.EngineFrontend`)."""
        return [self.speaker_bundle(p) for p in prompts]

    def emo_conds(self, prompts) -> List[torch.Tensor]:
        return [self.emo_cond(p) for p in prompts]

    def merge_emovec(self, spk_cond_emb, emo_cond_emb, alpha: float) -> torch.Tensor:   # gpt.merge_emovec (:759-765)
        raise NotImplementedError

    def emo_vector_mix(self, emo_vector, style, use_random: bool):  # (:669-680) -> (emovec_mat (1,D), weight_sum)
        raise NotImplementedError

    def text_segments(self, text: str, lang: str, max_text_tokens_per_segment: int, text_normalization: bool,
                      capacity: int) -> List[torch.Tensor]:
        """normalise, split (split_text_by_tokens :427-464), tokenize `<|lang|> seg`, append the stop id (:699-727)."""
        raise NotImplementedError

    def lang_id(self, lang: str) -> int:
        raise NotImplementedError

    def codes_to_mel(self, codes: torch.Tensor, code_lens: torch.Tensor, bundle, duration_factor: float):
        """semantic_codec.decode -> length_regulator -> cfm.inference -> drop prompt frames (:830-846).
        -> mel (B, 80, Tmax) f32 and lens (B,) frames."""
        raise NotImplementedError


class IndexTTS2:
    USE_GPT_LATENT = False                 # the s2mel stage of IndexTTS-2 carries the GPT-latent projector `gpt_layer` (subclass sets it)
    SPK_COND_MODE = "campplus"             # `UnifiedVoice(..., spk_cond_mode=)` of this version (infer_v2_5.py:106; v2: the default, conformer)
    # `infer_requests(prompt_batching=)`'s default (settable per object): encode the cold prompts of a call in ONE ragged prompt-side pass
    # (`Frontend.speaker_bundles`).  Off: a bundle encoded in a batch may differ from the bundle encoded alone in the last bits
    prompt_batching = False

    @staticmethod
    def _bigvgan_dir(model_dir, aux_paths=None):
        """infer_v2_5.py:224-228: `<model_dir>/hf_cache/bigvgan`, else the pre-downloaded `aux_paths["bigvgan"]`."""
        d = os.path.join(model_dir, "hf_cache", "bigvgan")
        if not os.path.isdir(d) and aux_paths and "bigvgan" in aux_paths:
            d = aux_paths["bigvgan"]
        return d

    def __init__(self, cfg_path="checkpoints/config.yaml", model_dir="checkpoints", use_bf16=False, device=None,
                 use_cuda_kernel=None, use_deepspeed=False, use_accel=False, use_torch_compile=False, use_qwen_emo=False,
                 *, frontend: Optional[Frontend] = None, gpt=None, bigvgan=None, cfg: Optional[dict] = None,
                 semantic_codec=None, s2mel=None, aux_paths=None, codes_to_mel="auto"):
        """`codes_to_mel`: where codes -> mel runs.  "engine": the HIP codec / length regulator / CFM stages (given as
        `semantic_codec=` / `s2mel=` or built from the frontend's state dicts) -- raises if they cannot be built; "frontend": the
        frontend's PyTorch `codes_to_mel` (north_star keeps s2mel on PyTorch as a legitimate integration mode); "auto" (default):
        the engine when its stages are available, else the frontend, and the choice is recorded in `self.codes_to_mel_mode`."""
        if codes_to_mel not in ("auto", "engine", "frontend"):
            raise ValueError(f"codes_to_mel must be 'auto', 'engine' or 'frontend', got {codes_to_mel!r}")
        if device is not None:
            self.device = device
        elif torch.cuda.is_available():
            self.device = "cuda:0"
        else:
            raise RuntimeError("IndexTTS2 (HIP engine) needs a GPU: there is no CPU path")
        self.use_bf16 = bool(use_bf16)
        self.use_cuda_kernel = True            # the HIP kernels are the only implementation
        self.model_dir = model_dir
        self.dtype = torch.bfloat16 if self.use_bf16 else None
        if cfg is None:
            import yaml
            with open(cfg_path) as f:
                cfg = yaml.safe_load(f)
        self.cfg = cfg
        gcfg = dict(cfg["gpt"])
        self.stop_mel_token = gcfg.get("stop_mel_token", 8193)
        self.model_version = cfg.get("version", None)
        self.gr_progress = None
        self.low_vram = False                  # infer_v2_5.py:124-131 turns it on below 10 GB of device memory; callers may set it
        self.qwen_emo = None
        if use_qwen_emo:
            raise NotImplementedError("QwenEmotion (text -> emotion vector) is a prompt-side LLM; run it with the reference "
                                      "package and pass emo_vector= instead")
        if gpt is None:
            from .gpt import UnifiedVoice
            gcfg.pop("spk_cond_mode", None)
            gpt = UnifiedVoice(**gcfg, spk_cond_mode=self.SPK_COND_MODE, precision="bf16" if self.use_bf16 else "fp32",
                               device=self.device)
            ck = torch.load(os.path.join(model_dir, cfg["gpt_checkpoint"]), map_location="cpu")
            gpt.load_state_dict(ck["model"] if "model" in ck else ck)
            gpt.post_init_gpt2_config(use_deepspeed=False, kv_cache=True, half=self.use_bf16)
        self.gpt = gpt
        if bigvgan is None:
            from .bigvgan import BigVGAN
            bigvgan = BigVGAN.from_pretrained(self._bigvgan_dir(model_dir, aux_paths)).to(self.device)
        self.bigvgan = bigvgan
        # codes -> mel on the HIP engine when both stages are given (indextts_amd.codec.EnhancedCodec, indextts_amd.s2mel.MyModel);
        # otherwise the frontend's codes_to_mel (the reference's PyTorch modules) is used
        self.semantic_codec = semantic_codec
        self.s2mel = s2mel
        if frontend is None:
            frontend = ReferenceFrontend(cfg, model_dir, self.device, self.gpt, cfg_path=cfg_path)
        self.frontend = frontend
        if codes_to_mel == "frontend":
            self.semantic_codec = self.s2mel = None
        elif (self.s2mel is None or self.semantic_codec is None) and hasattr(frontend, "engine_state_dicts") and "s2mel" in cfg \
                and "semantic_codec" in cfg:
            # codes -> mel on the engine, weights from the state dicts the frontend read (the reference's modules, or codec.pth / s2mel.pth
            # themselves); a stage that was injected is kept
            from .codec import EnhancedCodec
            from .s2mel import MyModel
            sds = frontend.engine_state_dicts()
            if self.semantic_codec is None:
                self.semantic_codec = EnhancedCodec(**dict(cfg["semantic_codec"]), device=self.device)
                self.semantic_codec.load_state_dict(sds["semantic_codec"])
            if self.s2mel is None:
                net = {"cfm": sds["cfm"], "length_regulator": sds["length_regulator"]}
                if self.USE_GPT_LATENT:                   # IndexTTS-2: MyModel(cfg.s2mel, use_gpt_latent=True), infer_v2.py:145
                    if "gpt_layer" not in sds:
                        raise RuntimeError("IndexTTS-2 needs the s2mel checkpoint's `gpt_layer` (latent projector): this frontend's "
                                           "engine_state_dicts() has none -- use indextts_amd.frontend.EngineFrontendV2 or inject s2mel=")
                    net["gpt_layer"] = sds["gpt_layer"]
                self.s2mel = MyModel(cfg["s2mel"], use_gpt_latent=self.USE_GPT_LATENT, precision="bf16" if self.use_bf16 else "fp32",
                                     device=self.device)
                self.s2mel.load_state_dict(net)
        if codes_to_mel == "engine" and (self.s2mel is None or self.semantic_codec is None):
            raise RuntimeError("codes_to_mel='engine': the HIP codec / s2mel stages were neither injected (semantic_codec=, s2mel=) nor "
                               "buildable from this frontend (it needs engine_state_dicts() and cfg['s2mel'] / cfg['semantic_codec'])")
        self.codes_to_mel_mode = "engine" if (self.s2mel is not None and self.semantic_codec is not None) else "frontend"
        self.tokenizer = getattr(frontend, "tokenizer", None)
        # reference cache attributes (:269-279)
        self.cache_spk_cond = None
        self.cache_s2mel_style = None
        self.cache_s2mel_prompt = None
        self.cache_spk_audio_prompt = None
        self.cache_emo_cond = None
        self.cache_emo_audio_prompt = None
        self.cache_mel = None
        self._bundle = None
        self.last_timing = {}
        self.last_scores = None                # `infer_requests` with best_of > 1 / token_scores=True: per request and segment, the candidates' scores
        self.alignment_heads = None            # [(layer, head), ...] `infer_requests(timestamps=True)` reads the text attention of (no default
                                               # list is shipped: no checkpoint's heads have been ranked; `TokenAlignment.monotonicity` ranks them)
        self.last_timestamps = None            # `infer_requests(timestamps=True)`: per request and segment, [dict(text_id, start, end)] in seconds
        self.last_loudness = None              # `audio_format` with `loudness_lufs`: per request dict(measured_lufs, gain_db, peak_dbfs_after), None
                                               # for the requests whose format names no loudness
        self.last_limiter = None               # `audio_format` with `limit_dbfs`: per request dict(max_reduction_db, peak_dbfs_after), None for the
                                               # requests whose format names no limiter
        # mixed-voice batches (`infer_requests`): every distinct speaker / emotion prompt is encoded once and kept (LRU); the single-entry
        # cache attributes above stay what `infer` / `infer_batch` use
        from .serving import SpeakerCache
        self.speaker_cache = SpeakerCache(lambda a: self.frontend.speaker_bundle(a))
        self.emotion_cache = SpeakerCache(lambda a: self.frontend.emo_cond(a))

    # ---- helpers mirrored from the reference ---------------------------------------------------------------------
    def _set_gr_progress(self, value, desc):
        if self.gr_progress is not None:
            self.gr_progress(value, desc=desc)

    def interval_silence(self, wavs, sampling_rate=22050, interval_silence=200):
        if not wavs or interval_silence <= 0:
            return wavs
        return torch.zeros(wavs[0].size(0), int(sampling_rate * interval_silence / 1000.0))

    def insert_interval_silence(self, wavs, sampling_rate=22050, interval_silence=200):
        if not wavs or interval_silence <= 0:
            return wavs
        sil = torch.zeros(wavs[0].size(0), int(sampling_rate * interval_silence / 1000.0))
        out = []
        for i, w in enumerate(wavs):
            out.append(w)
            if i < len(wavs) - 1:
                out.append(sil)
        return out

    def trim_codes(self, codes: torch.Tensor):
        """Stop-token trim (:809-821): per row the length up to the first stop token, batch cut to the longest."""
        lens = []
        for code in codes:
            hit = (code == self.stop_mel_token).nonzero(as_tuple=False)
            lens.append(int(hit[0, 0]) if hit.numel() > 0 else int(code.numel()))
        mx = max(lens) if lens else 0
        return codes[:, :mx], torch.tensor(lens, dtype=torch.long, device=codes.device)

    # ---- conditioning --------------------------------------------------------------------------------------------
    def _speaker(self, spk_audio_prompt):
        if self._bundle is None or self.cache_spk_audio_prompt != spk_audio_prompt:
            self._bundle = self.frontend.speaker_bundle(spk_audio_prompt)
            self.cache_spk_audio_prompt = spk_audio_prompt
            self.cache_spk_cond = self._bundle["spk_cond_emb"]
            self.cache_s2mel_style = self._bundle["style"]
            self.cache_s2mel_prompt = self._bundle["prompt_condition"]
            self.cache_mel = self._bundle["ref_mel"]
        return self._bundle

    def _emotion(self, emo_audio_prompt):
        if self.cache_emo_cond is None or self.cache_emo_audio_prompt != emo_audio_prompt:
            self.cache_emo_cond = self.frontend.emo_cond(emo_audio_prompt)
            self.cache_emo_audio_prompt = emo_audio_prompt
        return self.cache_emo_cond

    def _emovec(self, bundle, emo_audio_prompt, emo_alpha, emo_vector, use_random, emo_cond_emb=None):
        if emo_cond_emb is None:
            emo_cond_emb = self._emotion(emo_audio_prompt)
        if getattr(self.gpt, "cond_encoders", None) is not None:      # emotion Conformer + Perceiver on the engine (indextts_amd/cond.py)
            spk = bundle["spk_cond_emb"]
            # the reference passes the feature WIDTH (1024) as the "length" (:760-765): every frame of a
            # prompt shorter than 1024 frames is valid, a longer one is cut there
            emovec = self.gpt.merge_emovec(spk, emo_cond_emb, torch.tensor([min(spk.shape[-1], spk.shape[1])]),
                                           torch.tensor([min(emo_cond_emb.shape[-1], emo_cond_emb.shape[1])]), alpha=emo_alpha)
        else:
            emovec = self.frontend.merge_emovec(bundle["spk_cond_emb"], emo_cond_emb, emo_alpha)
        if emo_vector is not None:
            emovec_mat, wsum = self.frontend.emo_vector_mix(emo_vector, bundle["style"], use_random)
            emovec = emovec_mat + (1 - wsum) * emovec                 # (:767-769)
        return emovec

    # ---- API -------------------------------------------------------------------------------------------------------
    @staticmethod
    def split_text_by_punctuation(text, max_chars=40):
        """infer_v2_5.py:466-487: pieces of at most `max_chars` characters cut after punctuation; a piece with no punctuation
        stays whole (no mid-word cut)."""
        import re
        pieces, cur = [], ""
        for part in re.split(r'(?<=[\uff0c\u3002\uff01\uff1f\u3001\uff1b\uff1a,\.!\?;:\n])', text):
            if not part:
                continue
            if len(cur) + len(part) <= max_chars:
                cur += part
            else:
                if cur:
                    pieces.append(cur)
                cur = part
        if cur:
            pieces.append(cur)
        return pieces

    def _infer_low_vram(self, run_piece, text, output_path, interval_silence, verbose):
        """The `low_vram` branch of `infer()` (infer_v2_5.py:510-547; a < 10 GB device there, never an MI355X: `self.low_vram` is False
        unless the caller sets it): the text is cut at punctuation into <= 40-character pieces, each synthesised by its own
        `infer_generator` call with no inner silence, the int16 results joined with `interval_silence` ms of zeros."""
        pieces = self.split_text_by_punctuation(text, max_chars=40)
        if verbose:
            print(f">> Low-VRAM: split into {len(pieces)} segments: {pieces}")
        sr, wavs = 22050, []
        for piece in pieces:
            result = None
            for result in run_piece(piece):
                pass
            if result is not None and isinstance(result, tuple):
                wavs.append(torch.from_numpy(result[1].T).to(torch.int16))
        if not wavs:
            return None
        sil = torch.zeros(1, int(sr * interval_silence / 1000), dtype=torch.int16)
        parts = []
        for i, w in enumerate(wavs):
            parts.append(w)
            if i < len(wavs) - 1:
                parts.append(sil)
        wav = torch.cat(parts, dim=1)
        if output_path:
            if os.path.isfile(output_path):
                os.remove(output_path)
            if os.path.dirname(output_path) != "":
                os.makedirs(os.path.dirname(output_path), exist_ok=True)
            save_pcm_wav(output_path, wav, sr)
            return output_path
        return (sr, wav.numpy().T)

    def infer(self, spk_audio_prompt, text, output_path, lang, emo_audio_prompt=None, emo_alpha=1.0, emo_vector=None,
              use_emo_text=False, emo_text=None, use_random=False, interval_silence=200, verbose=False,
              max_text_tokens_per_segment=120, stream_return=False, more_segment_before=0, duration_factor=1.0,
              text_normalization=True, **generation_kwargs):
        from .output import refuse_audio_format
        refuse_audio_format(generation_kwargs, "infer")
        if getattr(self, "low_vram", False) and not stream_return and len(text) > 40:
            return self._infer_low_vram(
                lambda piece: self.infer_generator(spk_audio_prompt, piece, None, lang, emo_audio_prompt, emo_alpha, emo_vector,
                                                   use_emo_text, emo_text, use_random, 0, verbose, max_text_tokens_per_segment, False, 0,
                                                   duration_factor=duration_factor, text_normalization=text_normalization,
                                                   **generation_kwargs),
                text, output_path, interval_silence, verbose)
        gen = self.infer_generator(spk_audio_prompt, text, output_path, lang, emo_audio_prompt, emo_alpha, emo_vector,
                                   use_emo_text, emo_text, use_random, interval_silence, verbose,
                                   max_text_tokens_per_segment, stream_return, more_segment_before, duration_factor,
                                   text_normalization, **generation_kwargs)
        if stream_return:
            return gen
        try:
            return list(gen)[0]
        except IndexError:
            return None

    def infer_generator(self, spk_audio_prompt, text, output_path, lang, emo_audio_prompt=None, emo_alpha=1.0,
                        emo_vector=None, use_emo_text=False, emo_text=None, use_random=False, interval_silence=200,
                        verbose=False, max_text_tokens_per_segment=120, stream_return=False, quick_streaming_tokens=0,
                        duration_factor=1.0, text_normalization=True, **generation_kwargs):
        yield from self._infer_impl(spk_audio_prompt, text, output_path, lang, emo_audio_prompt, emo_alpha, emo_vector, use_emo_text,
                                    emo_text, use_random, interval_silence, verbose, max_text_tokens_per_segment, stream_return,
                                    duration_factor, text_normalization, generation_kwargs)

    def _infer_impl(self, spk_audio_prompt, text, output_path, lang, emo_audio_prompt, emo_alpha, emo_vector, use_emo_text, emo_text,
                    use_random, interval_silence, verbose, max_text_tokens_per_segment, stream_return, duration_factor,
                    text_normalization, generation_kwargs):
        """Body of `infer_generator` (infer_v2_5.py:570-899; infer_v2.py:396-720 has the same flow without `lang`, `duration_factor`
        and `text_normalization`: the v2 subclass passes lang=None, 1.0, True)."""
        from .output import refuse_audio_format
        refuse_audio_format(generation_kwargs, "infer / infer_generator")
        start_time = time.perf_counter()
        self._set_gr_progress(0, "starting inference...")
        if use_emo_text:
            raise RuntimeError("use_emo_text=True requires QwenEmotion, but it was not loaded at init "
                               "(use_qwen_emo=False). Re-construct IndexTTS2 with use_qwen_emo=True.")
        if emo_vector is not None:
            emo_audio_prompt = None
            scale = max(0.0, min(1.0, emo_alpha))
            if scale != 1.0:
                emo_vector = [int(x * scale * 10000) / 10000 for x in emo_vector]
        if emo_audio_prompt is None:
            emo_audio_prompt, emo_alpha = spk_audio_prompt, 1.0
        bundle = self._speaker(spk_audio_prompt)
        emovec = self._emovec(bundle, emo_audio_prompt, emo_alpha, emo_vector, use_random)
        self._set_gr_progress(0.1, "text processing...")
        capacity = self.gpt.n_text_pos
        segments = self.frontend.text_segments(text, lang, max_text_tokens_per_segment, text_normalization, capacity)
        if not segments:
            return
        sr = 22050
        lang_id = self.frontend.lang_id(lang) if lang is not None else 0
        wavs = self._synthesize(segments, [lang_id] * len(segments), bundle, emovec, duration_factor,
                                generation_kwargs, max_text_tokens_per_segment)
        silence = None
        if stream_return:
            for w in wavs:
                yield w
                if silence is None:
                    silence = self.interval_silence(wavs, sampling_rate=sr, interval_silence=interval_silence)
                yield silence
        end_time = time.perf_counter()
        self._set_gr_progress(0.9, "saving audio...")
        wav = torch.cat(self.insert_interval_silence(wavs, sampling_rate=sr, interval_silence=interval_silence), dim=1)
        wav_length = wav.shape[-1] / sr
        t = self.last_timing
        print(f">> gpt_gen_time: {t.get('gpt', 0):.2f} seconds")
        print(f">> s2mel_time: {t.get('s2mel', 0):.2f} seconds")
        print(f">> bigvgan_time: {t.get('bigvgan', 0):.2f} seconds")
        print(f">> Total inference time: {end_time - start_time:.2f} seconds")
        print(f">> Generated audio length: {wav_length:.2f} seconds")
        print(f">> RTF: {(end_time - start_time) / max(wav_length, 1e-9):.4f}")
        if output_path:
            if os.path.isfile(output_path):
                os.remove(output_path)
            if os.path.dirname(output_path) != "":
                os.makedirs(os.path.dirname(output_path), exist_ok=True)
            save_pcm_wav(output_path, wav, sr)
            if stream_return:
                return
            yield output_path
        else:
            if stream_return:
                return
            yield (sr, wav.type(torch.int16).numpy().T)

    def _audio_format(self, value, who: str):
        """`audio_format=` of a pipeline entry -> `output.AudioFormat`, None when none is given (the entry then runs the code it always ran).  A
        given one is a ValueError where the delivery stage does not run: under torch.distributed and in the IndexTTS-2 pipeline."""
        if value is None:
            return None
        from . import dist as D
        from .output import AudioFormat
        if D.world() > 1:
            raise ValueError(f"{who}: `audio_format` is not available under torch.distributed (the ranks' rows are gathered as int16)")
        if self.SPK_COND_MODE != "campplus":
            raise ValueError(f"{who}: `audio_format` is implemented for the IndexTTS-2.5 pipeline (campplus conditioning)")
        return AudioFormat.parse(value)

    def infer_batch(self, spk_audio_prompt, texts: Sequence[str], lang, emo_audio_prompt=None, emo_alpha=1.0,
                    interval_silence=200, max_text_tokens_per_segment=120, duration_factor=1.0, text_normalization=True,
                    **generation_kwargs):
        """New capability (BASELINE.json configs[1,2]): many utterances of one speaker in one pass.  Every segment of
        every utterance is a row of one GPT batch / one ragged BigVGAN batch.  Returns a list of (22050, int16 (T,1)).

        Under `torch.distributed` (one process per GPU, `indextts_amd.dist`) the segment rows are LPT-sharded over the ranks
        by text length: rank 0 runs the prompt encoders and broadcasts the speaker bundle (the one collective before the
        decode loop), every rank decodes and vocodes its own rows, the int16 waveforms are gathered on rank 0, which returns
        the full list; the other ranks return None per utterance.

        `cfm_noise="request"` (default "global": torch's generator): the flow-matching noise of row i is keyed by (the call's `seed`, i) -- the
        stream value the token draw of that row uses -- so the same call with the same seed gives the same audio, whatever was drawn before.
        Without a `seed` one is drawn from torch's generator, as `generate` draws its own.

        `audio_format=` (`output.AudioFormat`, a dict or "rate/encoding"; one process only): every utterance is assembled, resampled and encoded
        on the device (indextts_amd/output.py) and comes back as (the format's rate, (T, 1) array of the encoding's dtype)."""
        from . import dist as D
        from .gpt import refuse_code_prefix
        generation_kwargs = dict(generation_kwargs)
        fmt = self._audio_format(generation_kwargs.pop("audio_format", None), "infer_batch")
        self._cfm_noise_mode(dict(generation_kwargs))            # an unknown value fails before any work
        refuse_code_prefix(generation_kwargs, "infer_batch")
        world, rank = D.world(), D.rank()
        if emo_audio_prompt is None:
            emo_audio_prompt, emo_alpha = spk_audio_prompt, 1.0
        bundle = None
        if rank == 0:
            bundle = dict(self._speaker(spk_audio_prompt))
            bundle["emo_vec"] = self._emovec(bundle, emo_audio_prompt, emo_alpha, None, False)
        if world > 1:
            bundle = D.broadcast_speaker_bundle(bundle, src=0, device=self.device)
        emovec = bundle["emo_vec"]
        capacity = self.gpt.n_text_pos
        seg_tokens, owner = [], []
        for u, text in enumerate(texts):                    # tokenisation is deterministic host work: every rank does it
            segs = self.frontend.text_segments(text, lang, max_text_tokens_per_segment, text_normalization, capacity)
            seg_tokens += segs
            owner += [u] * len(segs)
        if not seg_tokens:
            return [None] * len(texts)
        mine = D.shard_utterances(len(seg_tokens), rank, world, lengths=[int(t.numel()) for t in seg_tokens]) if world > 1 \
            else list(range(len(seg_tokens)))
        if fmt is not None:                                  # (one process: every row is mine) the rows stay on the device, in [-1, 1]
            from . import output
            rows, lens = self._synthesize(seg_tokens, [self.frontend.lang_id(lang)] * len(seg_tokens), bundle, emovec, duration_factor,
                                          generation_kwargs, max_text_tokens_per_segment, device_rows=True)
            groups = [[i for i, o in enumerate(owner) if o == u] for u in range(len(texts))]
            full = [u for u, g in enumerate(groups) if g]
            out, measured, limited = [None] * len(texts), [], []
            self.last_loudness, self.last_limiter = [None] * len(texts), [None] * len(texts)
            arrays = output.convert(rows, lens, [groups[u] for u in full], fmt, interval_silence, report=measured, limiter_report=limited)
            for u, a, m, lim in zip(full, arrays, measured, limited):
                out[u] = (fmt.sample_rate, a.reshape(-1, 1))
                self.last_loudness[u], self.last_limiter[u] = m, lim
            return out
        wavs = []
        if mine:
            wavs = self._synthesize([seg_tokens[i] for i in mine], [self.frontend.lang_id(lang)] * len(mine), bundle, emovec,
                                    duration_factor, generation_kwargs, max_text_tokens_per_segment)
        if world > 1:
            wavs = D.gather_waveforms([w.type(torch.int16) for w in wavs], mine, len(seg_tokens), dst=0)
            if rank != 0:
                return [None] * len(texts)
            wavs = [w.float() for w in wavs]                 # int16 -> float is exact; silence is inserted in float
        out = []
        for u in range(len(texts)):
            seg = [w for w, o in zip(wavs, owner) if o == u]
            if not seg:
                out.append(None)
                continue
            wav = torch.cat(self.insert_interval_silence(seg, 22050, interval_silence), dim=1)
            out.append((22050, wav.type(torch.int16).numpy().T))
        return out

    def infer_stream(self, spk_audio_prompt, texts: Sequence[str], lang, emo_audio_prompt=None, emo_alpha=1.0, chunk_size: int = 100,
                     overlap_size: int = 20, max_text_tokens_per_segment=120, duration_factor=1.0, text_normalization=True,
                     **generation_kwargs):
        """Streaming synthesis of a batch of single-segment texts (`FasterIndexTTS2` streaming path,
        backends/trt/pipeline/streaming.py): a generator of `(22050, [int16 array | None per text], [done per text])`, one item per
        GPT chunk of `chunk_size` codes (consecutive chunks share `overlap_size` codes and are cross-faded).  The first audio
        leaves after prefill + `chunk_size` decode steps + one chunk of codes -> mel -> waveform instead of after the whole
        utterance.  Sampling uses one hypothesis per row (`num_beams` is forced to 1: a beam's prefix is not final mid-search).
        `cfm_noise="request"`: the flow-matching noise of chunk k of row i is keyed by (`seed`, i, chunk = k), so a stream run twice with one seed
        is the same audio (default "global": torch's generator).
        `audio_format=` (`output.AudioFormat`, a dict or "rate/encoding"; no `peak_dbfs`): the items are `(the format's rate, [array of the
        encoding's dtype | None], [done])`; cross-fade, resampling and encoding of all rows run on the device (`output.deliver`).  With
        `AudioFormat()` a piece is within 1 LSB of the piece without the kwarg (rounding instead of truncation, f32 window tables)."""
        from .streaming import StreamingDecoder
        from .output import stream_format
        gk = dict(generation_kwargs)
        fmt = stream_format(self._audio_format(gk.pop("audio_format", None), "infer_stream"), "infer_stream")
        self._refuse_timestamps(gk, "infer_stream")
        from .gpt import refuse_code_prefix
        refuse_code_prefix(gk, "infer_stream")
        keyed = self._cfm_noise_mode(gk) == "request"
        if keyed:
            self._need_engine_s2mel("cfm_noise='request'")
            if gk.get("seed") is None:
                gk["seed"] = self.gpt._seed(None, True, None)
        if emo_audio_prompt is None:
            emo_audio_prompt, emo_alpha = spk_audio_prompt, 1.0
        bundle = dict(self._speaker(spk_audio_prompt))
        emovec = self._emovec(bundle, emo_audio_prompt, emo_alpha, None, False)
        seg_tokens = []
        for text in texts:
            segs = self.frontend.text_segments(text, lang, max_text_tokens_per_segment, text_normalization, self.gpt.n_text_pos)
            if len(segs) != 1:
                raise ValueError("infer_stream takes texts of one segment each (split long texts with the frontend first)")
            seg_tokens.append(segs[0])
        gk.pop("do_sample", None)
        gk.pop("num_beams", None)
        max_mel_tokens = gk.pop("max_mel_tokens", 1500)
        gen = dict(do_sample=True, top_p=gk.pop("top_p", 0.8), top_k=gk.pop("top_k", 30), temperature=gk.pop("temperature", 0.8),
                   repetition_penalty=gk.pop("repetition_penalty", 10.0), length_penalty=gk.pop("length_penalty", 0.0), num_beams=1, **gk)
        dev = self.device
        L = max(int(t.numel()) for t in seg_tokens)
        text_ids = torch.full((len(seg_tokens), L), 1, dtype=torch.int32)
        for i, t in enumerate(seg_tokens):
            text_ids[i, : t.numel()] = t.reshape(-1).to(torch.int32)
        langs = torch.tensor([self.frontend.lang_id(lang)] * len(seg_tokens), dtype=torch.long)
        inputs_embeds, attention_mask, max_new, hf = self.gpt.inference_speech_stream(
            bundle["spk_cond_emb"], text_ids.to(dev), chunk_size, overlap_size, langs=langs.to(dev), emo_vec=emovec,
            campplus_embedding=bundle["style"], max_generate_length=max_mel_tokens, **gen)
        up = self.bigvgan.total_up

        def codes_to_audio(codes, code_lens):
            lens = torch.as_tensor(code_lens).to(torch.int32).cpu().clamp(min=1)          # finished rows render one frame pair, dropped by the decoder
            if self.s2mel is not None and self.semantic_codec is not None:
                n = codes.shape[0]
                s2kw = dict(noise_keys=([int(gen["seed"])] * n, list(range(n)), [dec.chunk_index] * n)) if keyed else {}      # (seed, row, chunk)
                mel, mel_lens = self.codes_to_mel(codes, lens, bundle, duration_factor, **s2kw)
            else:
                mel, mel_lens = self.frontend.codes_to_mel(codes, lens, bundle, duration_factor)
            wav = self.bigvgan(mel.float(), lens=mel_lens)
            if fmt is not None:                            # the rows stay on the device: `output.deliver` makes the pieces there
                return [wav[i, 0, : int(mel_lens[i]) * up].float() for i in range(wav.shape[0])]
            return [wav[i, 0, : int(mel_lens[i]) * up].float().cpu().numpy() for i in range(wav.shape[0])]

        # the cross-fade spans the samples the overlapping codes render to: int(2 * n * 1.72 * duration_factor) frames for n codes here
        # (infer_v2_5.py:833), not the reference decoder's fixed 1.72 frames per code of IndexTTS-2
        dec = StreamingDecoder(self.gpt, codes_to_audio, chunk_size=chunk_size, overlap_size=overlap_size,
                               frames_per_code=2 * 1.72 * float(duration_factor), audio_format=fmt)
        self.last_stream = dec
        yield from dec.generate(inputs_embeds, attention_mask, max_new, **hf)

    def codes_to_mel(self, codes: torch.Tensor, code_lens: torch.Tensor, bundle, duration_factor: float = 1.0,
                     diffusion_steps=25, inference_cfg_rate=0.7, noise: Optional[torch.Tensor] = None, bundle_index=None, noise_keys=None,
                     noise_temperature=1.0):
        """infer_v2_5.py:830-846 for a whole batch of segments on the HIP engine: semantic_codec.decode -> length_regulator ->
        [prompt_condition | cond] -> cfm.inference -> drop the prompt frames.  Every row is processed at its own lengths (what the
        reference's batch-1 call per segment computes).  Mixed voices: `bundle` a list of bundles, `bundle_index` the bundle of every row
        (`s2mel.codes_to_mel`).  `noise_keys=(seeds, streams[, chunks])` per row: seeded, batch-invariant flow-matching noise instead of torch's
        generator; `noise_temperature`, `diffusion_steps` and `inference_cfg_rate` may be one value per row.  Returns mel (B, 80, max frames) f32
        and the frame counts (B,) int32."""
        from .s2mel import codes_to_mel
        return codes_to_mel(self.semantic_codec, self.s2mel.models, codes, code_lens, bundle, duration_factor, diffusion_steps,
                            inference_cfg_rate, noise, bundle_index=bundle_index, noise_keys=noise_keys, noise_temperature=noise_temperature)

    @staticmethod
    def _cfm_noise_mode(kwargs: dict) -> str:
        """pops `cfm_noise` from a call's keyword arguments: "global" (the default: torch's generator, as the reference draws the flow-matching
        noise) or "request" (keyed by the request's seed and stream: `CFM.inference(noise_keys=)`)"""
        mode = kwargs.pop("cfm_noise", "global")
        if mode not in ("global", "request"):
            raise ValueError(f"cfm_noise must be 'global' or 'request', got {mode!r}")
        return mode

    def _need_engine_s2mel(self, what: str):
        if self.s2mel is None or self.semantic_codec is None:
            raise ValueError(f"{what} needs the engine's codec / s2mel stages (codes_to_mel='engine'); the frontend's PyTorch codes_to_mel "
                             "draws its noise from torch's generator at fixed settings")

    # ---- mixed-request batches: per-row voices and per-row sampling settings -------------------------------------------------------------
    _REQUEST_KEYS = frozenset(("spk_audio_prompt", "text", "lang", "emo_audio_prompt", "emo_alpha", "emo_vector", "duration_factor", "top_p", "top_k",
                               "temperature", "repetition_penalty", "max_mel_tokens", "seed", "typical_sampling", "typical_mass",
                               "diffusion_steps", "inference_cfg_rate", "cfm_temperature", "best_of"))
    _REQUEST_S2MEL = dict(diffusion_steps=25, inference_cfg_rate=0.7, cfm_temperature=1.0)      # codes -> mel settings of a request and their defaults
    _REQUEST_SAMPLING = ("top_p", "top_k", "temperature", "repetition_penalty", "max_mel_tokens", "seed", "typical_sampling", "typical_mass")

    @staticmethod
    def _request_filters(req: dict) -> dict:
        """a request's own logits-filter keys (`gpt._LOGITS_FILTER_KWARGS`), as an entry of `generate(row_filters=)`: a key the request HAS
        wins over the call's value, whatever it holds"""
        from .gpt import _LOGITS_FILTER_KWARGS
        return {k: req[k] for k in _LOGITS_FILTER_KWARGS if k in req}

    @staticmethod
    def _refuse_timestamps(gk: dict, who: str) -> None:
        if gk.get("timestamps") or gk.get("alignment_heads") is not None:
            raise ValueError(f"{who}: timestamps / alignment_heads are implemented for infer_requests only (a stream's chunks are cross-faded "
                             "and leave before the row's alignment is complete)")

    @staticmethod
    def _rescore_flag(gk: dict, key: str) -> bool:
        """`timestamps` / `token_scores` of `infer_requests` given as a string: "rescore" (taken out of `gk`: -> True) is the only one"""
        v = gk.get(key)
        if not isinstance(v, str):
            return False
        if v != "rescore":
            raise ValueError(f"infer_requests: {key}={v!r}: the accepted values are True and 'rescore'")
        del gk[key]
        return True

    @staticmethod
    def segment_timestamps(spans, text_ids, n_codes: int, samples: int, samples_per_code: float, offset: int = 0, rate: int = 22050) -> list:
        """Per-token times of one rendered segment.  spans: (T, 2) [start_code, end_code) per text position of `[start][ids][stop]`
        (`TokenAlignment.path`), T = len(text_ids) + 2; code i starts at sample i * samples_per_code (2 * 1.72 * duration_factor frames of
        `bigvgan.total_up` samples: the rule `codes_to_mel` stretches by), clipped at the segment's `samples`; `offset`: the samples of the
        request's waveform before this segment.  The start token's codes go to the first id, the stop token's to the last, so the entries
        cover the segment: -> [dict(text_id, start, end)] in seconds, non-decreasing."""
        ids = [int(v) for v in text_ids]
        if not ids:
            return []
        at = lambda i: min(float(samples), max(0.0, int(i) * float(samples_per_code)))
        sp = [(int(a), int(b)) for a, b in (spans.tolist() if hasattr(spans, "tolist") else spans)]
        out, prev = [], 0.0
        for j, tid in enumerate(ids, start=1):
            a = 0.0 if j == 1 else max(prev, at(min(sp[j][0], n_codes)))
            b = float(samples) if j == len(ids) else max(a, at(min(sp[j][1], n_codes)))
            out.append(dict(text_id=tid, start=(offset + a) / float(rate), end=(offset + b) / float(rate)))
            prev = b
        return out

    def code_index_at(self, seconds: float, duration_factor: float = 1.0, rate: int = 22050) -> int:
        """The inverse of `segment_timestamps`' sample rule, to turn a time inside a rendered segment into a cut point for `code_prefix`:
        code i starts at sample i * 2 * 1.72 * duration_factor * `bigvgan.total_up`, so the code that is sounding at `seconds` after the
        segment's start is the last i whose start is <= it: -> that i (>= 0).  The codes before the cut are codes[:i]."""
        per_code = 2 * 1.72 * float(duration_factor) * int(self.bigvgan.total_up)
        if not (float(seconds) >= 0.0 and per_code > 0.0):
            raise ValueError(f"code_index_at: seconds >= 0 and duration_factor > 0, got {seconds}, {duration_factor}")
        i = int(float(seconds) * int(rate) / per_code)
        while (i + 1) * per_code <= float(seconds) * int(rate):      # (the float quotient may land one below at an exact boundary)
            i += 1
        while i > 0 and i * per_code > float(seconds) * int(rate):
            i -= 1
        return i

    @staticmethod
    def _request_prefix(r: int, value, n_segs: int) -> list:
        """The request key `code_prefix` -> one entry per segment (a list of ints, or None): one sequence or None per segment; a request of one
        segment may give its sequence bare.  The codes themselves are checked by the engine's host side (`UnifiedVoice._code_prefix`)."""
        if value is None:
            return [None] * n_segs
        as_list = lambda v: None if v is None else [int(x) for x in (v.reshape(-1).tolist() if hasattr(v, "reshape") else v)]
        bare = hasattr(value, "dim") and value.dim() == 1 or (isinstance(value, (list, tuple)) and len(value) > 0 and
                                                              all(isinstance(x, int) and not isinstance(x, bool) for x in value))
        if bare:
            value = [value]
        if not isinstance(value, (list, tuple)) or len(value) != n_segs:
            raise ValueError(f"request {r}: `code_prefix` has to hold one code sequence (or None) per segment ({n_segs}), got "
                             f"{len(value) if isinstance(value, (list, tuple)) else type(value).__name__}")
        return [as_list(v) for v in value]

    @staticmethod
    def _best_of(value, who: str) -> int:
        """`best_of` of a request or of the call's defaults: an int >= 1 (None: 1)"""
        if value is None:
            return 1
        if isinstance(value, bool) or not isinstance(value, int) or value < 1:
            raise ValueError(f"{who}: `best_of` has to be an int >= 1, but is {value!r}")
        return int(value)

    @staticmethod
    def _choose_candidate(mean_logprob, ended) -> int:
        """The `best_of` selection rule: candidates whose stop token was the model's own before those that ran into their cap, among those the
        greatest mean log-probability under the model's own distribution (nan -- no token of its own -- counts as -inf), ties to the lowest index"""
        key = lambda c: (bool(ended[c]), float(mean_logprob[c]) if float(mean_logprob[c]) == float(mean_logprob[c]) else float("-inf"))
        best = 0
        for c in range(1, len(ended)):
            if key(c) > key(best):
                best = c
        return best

    def _request_settings(self, r, req: dict, request_keys, s2_base: dict, base: dict) -> dict:
        """A request's normalised settings (`infer_requests`, `stream_session`): unknown keys are a ValueError, the sampling settings
        (`_REQUEST_SAMPLING`) and the codes -> mel settings (`_REQUEST_S2MEL`) are the request's own, else the call's (`base` / `s2_base`), else
        the pipeline's defaults, range-checked.  No device work."""
        unknown = sorted(set(req) - request_keys)
        if unknown:
            raise ValueError(f"request {r}: unknown keys {unknown}")
        given = {k: (req[k] if req.get(k) is not None else s2_base[k]) for k in self._REQUEST_S2MEL}
        if any(v is not None for v in given.values()):
            self._need_engine_s2mel(f"request {r}: {sorted(k for k, v in given.items() if v is not None)}")
        s2 = ({k: (self._REQUEST_S2MEL[k] if v is None else v) for k, v in given.items()})
        if int(s2["diffusion_steps"]) != s2["diffusion_steps"] or int(s2["diffusion_steps"]) < 1:
            raise ValueError(f"request {r}: `diffusion_steps` has to be an integer >= 1, but is {s2['diffusion_steps']}")
        if not 0.0 <= float(s2["inference_cfg_rate"]) < float("inf"):
            raise ValueError(f"request {r}: `inference_cfg_rate` has to be a float >= 0, but is {s2['inference_cfg_rate']}")
        if not 0.0 <= float(s2["cfm_temperature"]) < float("inf"):
            raise ValueError(f"request {r}: `cfm_temperature` has to be a float >= 0, but is {s2['cfm_temperature']}")
        st = {k: (req[k] if req.get(k) is not None else base[k]) for k in self._REQUEST_SAMPLING}
        if st["typical_sampling"] and not 0.0 < float(st["typical_mass"]) < 1.0:
            raise ValueError(f"request {r}: `typical_mass` has to be a float > 0 and < 1, but is {st['typical_mass']}")
        st.update(s2)
        st["best_of"] = self._best_of(req["best_of"] if req.get("best_of") is not None else base.get("best_of"), f"request {r}")
        return st

    def _request_conditioning(self, req: dict, bundles: list, bundle_of: dict, latents: dict):
        """A request's voice and emotion: -> (index of its speaker bundle in `bundles`, key of its conditioning latents (1, 3, D) in `latents`);
        every distinct prompt is encoded once (`self.speaker_cache` / `self.emotion_cache`), every distinct (voice, emotion) once per caller."""
        from .serving import SpeakerCache
        spk = req["spk_audio_prompt"]
        kb = SpeakerCache.key_of(spk)
        if kb not in bundle_of:
            bundle_of[kb] = len(bundles)
            bundles.append(self.speaker_cache.get_or_compute(spk))
        bi = bundle_of[kb]
        emo_prompt, emo_alpha, emo_vector = req.get("emo_audio_prompt"), float(req.get("emo_alpha", 1.0)), req.get("emo_vector")
        if emo_vector is not None:                     # as infer_generator (:592-600)
            emo_prompt = None
            scale = max(0.0, min(1.0, emo_alpha))
            if scale != 1.0:
                emo_vector = [int(x * scale * 10000) / 10000 for x in emo_vector]
        if emo_prompt is None:
            emo_prompt, emo_alpha = spk, 1.0
        kl = (bi, SpeakerCache.key_of(emo_prompt), emo_alpha, None if emo_vector is None else tuple(float(v) for v in emo_vector))
        if kl not in latents:
            emovec = self._emovec(bundles[bi], emo_prompt, emo_alpha, emo_vector, False,
                                  emo_cond_emb=self.emotion_cache.get_or_compute(emo_prompt))
            latents[kl] = self.gpt.conds_latent(bundles[bi]["style"], emovec)[0]
        return bi, kl

    def _warm_prompt_caches(self, requests: Sequence[dict]):
        """`prompt_batching=True`: the distinct speaker prompts of the call (first-appearance order) go through the front end's
        `speaker_bundles` as ONE list, the distinct emotion prompts (a request without one conditions on its speaker prompt, as
        `_request_conditioning` decides) through `emo_conds`; `_request_conditioning` then only hits the caches."""
        spk, emo = [], []
        for req in requests:
            spk.append(req["spk_audio_prompt"])
            emo_prompt = None if req.get("emo_vector") is not None else req.get("emo_audio_prompt")
            emo.append(req["spk_audio_prompt"] if emo_prompt is None else emo_prompt)
        self.speaker_cache.get_or_compute_many(spk, self.frontend.speaker_bundles)
        self.emotion_cache.get_or_compute_many(emo, self.frontend.emo_conds)

    def infer_requests(self, requests: Sequence[dict], interval_silence=200, max_text_tokens_per_segment=120, text_normalization=True,
                       **defaults):
        """Many requests with their OWN voice and their OWN sampling settings in one pass (per-request settings in one batch, as the
        reference's serving path keeps them: backends/trt/serving/triton_server.py:96-305).  A request is a dict: `spk_audio_prompt`, `text`,
        `lang`; optional `emo_audio_prompt`, `emo_alpha`, `emo_vector`, `duration_factor`; optional generation settings `top_p`, `top_k`,
        `temperature`, `repetition_penalty`, `max_mel_tokens`, `seed`, `typical_sampling`, `typical_mass`, `best_of` (missing: `**defaults`, then the
        pipeline's defaults), and the logits-filter kwargs `min_new_tokens`, `min_length`, `no_repeat_ngram_size`, `suppress_tokens`,
        `begin_suppress_tokens`, `bad_words_ids`, `exponential_decay_length_penalty`, `min_p`, `epsilon_cutoff`, `eta_cutoff` (a key the request
        has wins over the one in `**defaults`; all segments and all `best_of` candidates of a request share them).  When every request ends up
        with the same filters the call installs them call-wide, as it always did; otherwise every row gets its own record
        (`UnifiedVoice.generate(row_filters=)` at num_beams = 1, `group_filters=` with `beam_settings="own"`; with shared beam settings
        differing filters are a ValueError), and a request decodes as it does alone with its filters.  Call-wide (`**defaults` only): `num_beams`, `beam_settings`, `length_penalty` (a request key too with
        `beam_settings="own"`), `inflight_slots`, `inflight_beam_slots`, `chunk_tokens`, `min_free`.  Every segment of every request is a row of ONE GPT batch, one `codes_to_mel` call and one ragged vocoder
        batch; every distinct prompt is encoded once (`self.speaker_cache`).  Returns one (22050, int16 (T, 1)) per request, in request order.

        num_beams = 1: the rows' sampling settings go into the engine's per-slot table (`UnifiedVoice.generate(row_sampling=)`), the random
        stream of a row is keyed by (the request's seed, the segment's index in the request, the row's step) -- not by the slot -- so a
        request's codes do not depend on its slot or its batch mates: they are those of `infer_batch(voice, [text], seed=...)` of the request
        alone (this rests on the engine's batch invariance).  A request without a seed draws one from torch's generator.
        num_beams > 1 (the default 3), `beam_settings="shared"` (the default): requests may mix voices but must share the sampling settings
        (ValueError otherwise), and a beam-sampled request's codes depend on its slot and on the call's one seed.
        num_beams > 1, `beam_settings="own"`: every request keeps its own settings, `max_mel_tokens`, `seed` and `length_penalty` -- the rows'
        settings go into the beam kernels' per-group table (`UnifiedVoice.generate(group_sampling=, row_max_new=)`), the draw of a group is
        keyed by (the request's seed, the segment's index in the request, the group's own step), and a request gets the codes of
        `infer_batch(voice, [text], num_beams=..., seed=...)` of the request alone, as at num_beams = 1.

        `best_of` = N > 1 (num_beams = 1 only): every segment of the request decodes as N candidate rows of the same GPT batch -- candidate c of
        segment j draws from stream j + (c << 16), so candidate 0 is the row of a call without the key -- and only the winner is rendered: the
        candidates that ended with a stop token of their own before those that ran into their cap, among them the greatest mean per-token
        log-probability under the model's own distribution (`TokenScores.mean_logprob`), ties to the lowest c.  `last_scores[request][segment]`
        = dict(chosen, mean_logprob [N], lengths [N], ended [N]); `last_codes` holds the winners; with `token_scores=True` in `**defaults`
        the scores are kept at best_of = 1 too (chosen = 0).  Score bits are batch-invariant like the ids, so a request's chosen codes do not
        depend on its batch mates either.  Whether the highest mean log-probability picks the better-SOUNDING candidate has not been evaluated.

        `timestamps="rescore"` (with `alignment_heads=`) / `token_scores="rescore"`: any num_beams, shared or own beam settings, in-flight
        slots.  After decoding, the chosen codes of every segment go through ONE batched teacher-forced pass (`UnifiedVoice.rescore`):
        `last_timestamps` is filled as `timestamps=True` fills it (here row 0 of the attention is the start-mel query's, not zero) and
        `last_scores[request][segment]` = dict(mean_logprob, lengths) (beside a `best_of` report: the keys rescored_mean_logprob /
        rescored_lengths).  Codes and audio are those of the call without the kwarg.  `timestamps=True` / `token_scores=True` keep their
        meaning (the decode step's own export, num_beams = 1) and their refusals; any other string is a ValueError.

        `code_prefix` (a request key, num_beams = 1 only): one code sequence (or None) per segment of the request -- a request of one segment
        may give its sequence bare.  The segment's row continues after those codes (`UnifiedVoice.generate(code_prefix=)`): `last_codes` holds
        the FULL codes and the audio renders them, `max_mel_tokens` is the cap on the total.  With the request's original seed the
        continuation resumes the uninterrupted request (in exact arithmetic), in any slot and through
        `inflight_slots`; under `best_of` every candidate shares the prefix and candidate 0 is that resume; `token_scores=True` scores the
        generated columns only, `timestamps="rescore"` runs over the full codes; `timestamps=True` raises (the decode export has no rows
        for given codes).  `code_index_at` turns a time of `last_timestamps` into a cut point.

        The audio: "alone" holds for the CODES above.  The flow-matching stage that turns codes into mel starts from noise, and with the default
        `cfm_noise="global"` (call-wide) that noise comes from torch's generator as one (rows, 80, widest row) draw -- a row's audio then depends on
        the batch, its slot and everything drawn before.  With `cfm_noise="request"` the noise of a row is keyed like its token draw -- (the
        request's seed, the segment's index in the request) at num_beams = 1 and with `beam_settings="own"`, (the call's seed, the row's slot) in
        the "shared" beam mode -- and a request gets the AUDIO of `infer_batch(voice, [text], seed=..., cfm_noise="request")` of the request alone,
        in any batch and any order.  It needs the engine's codec / s2mel stages.
        Optional codes -> mel settings of a request (or `**defaults`), in either noise mode, engine stages only: `diffusion_steps` (25),
        `inference_cfg_rate` (0.7), `cfm_temperature` (1.0, the scale of the noise); rows are grouped by equal (steps, rate) for the solve.

        `prompt_batching=True` (call-wide; default: the attribute `prompt_batching`, False): before the request loop the call's distinct cold
        speaker prompts are encoded by ONE `frontend.speaker_bundles(list)` call and its distinct emotion prompts by ONE `frontend.emo_conds(list)`
        (`SpeakerCache.get_or_compute_many`) instead of one front-end call per prompt.  Off by default: a bundle encoded in a batch may differ
        from the same bundle encoded alone in the last bits, and "a request gets the audio it gets alone" is bitwise.

        `audio_format` (call-wide, and a request key that wins over it; `output.AudioFormat`, a dict or "rate/encoding"): the request is
        delivered in that format -- assembled at 22050 Hz with its interval silences, resampled as ONE sequence, peak-normalised when the format
        asks, encoded, all on the device (indextts_amd/output.py), one device-to-host copy per format of the call -- and comes back as (the
        format's rate, (T, 1) array of the encoding's dtype), T = ceil(N * rate / 22050).  A request without a format is returned as it always
        was, bit for bit, whatever its batch mates ask for.  `last_timestamps` are seconds: they hold at any rate.
        A format with `loudness_lufs` is normalised to that integrated loudness (ITU-R BS.1770-4), measured on the device over the whole request
        at the delivery rate (`peak_dbfs` beside it is a ceiling); `last_loudness[request]` then holds dict(measured_lufs, gain_db,
        peak_dbfs_after), None for the other requests.  The request gets the same bytes alone, in any batch and in any order.
        A format with `limit_dbfs` puts a 5 ms look-ahead limiter behind the gain (`true_peak=True`: of the true peak, dBTP), so a loudness
        target and a ceiling are both met; `last_limiter[request]` then holds dict(max_reduction_db, peak_dbfs_after).  `measured_lufs` stays the
        measurement before the limiter."""
        from . import dist as D
        requests = list(requests)
        given_format = [r.get("audio_format") for r in requests if isinstance(r, dict)] + [defaults.get("audio_format")]
        call_format = None
        for value in given_format:                         # refused (or a bad value found) before anything else happens
            call_format = self._audio_format(value, "infer_requests")
        if D.world() > 1:
            raise NotImplementedError("infer_requests under torch.distributed: the speaker-bundle broadcast carries one speaker (use infer_batch)")
        if self.SPK_COND_MODE != "campplus":
            raise NotImplementedError("infer_requests is implemented for the IndexTTS-2.5 pipeline (campplus conditioning)")
        if not requests:
            return []
        gk = dict(defaults)
        gk.pop("audio_format", None)                       # (the last value of the loop above) never reaches the GPT
        formats = [self._audio_format(r.get("audio_format"), "infer_requests") or call_format for r in requests]
        gk.pop("do_sample", None)
        prompt_batching = gk.pop("prompt_batching", None)
        prompt_batching = bool(self.prompt_batching if prompt_batching is None else prompt_batching)
        keyed_noise = self._cfm_noise_mode(gk) == "request"
        if keyed_noise:
            self._need_engine_s2mel("cfm_noise='request'")
        s2_base = {k: gk.pop(k, None) for k in self._REQUEST_S2MEL}
        num_beams = int(gk.pop("num_beams", 3))
        length_penalty = gk.pop("length_penalty", 0.0)
        beam_settings = gk.pop("beam_settings", "shared")
        if beam_settings not in ("shared", "own"):
            raise ValueError(f"infer_requests: beam_settings must be 'shared' or 'own', got {beam_settings!r}")
        own_beams = num_beams > 1 and beam_settings == "own"
        from .gpt import refuse_code_prefix, _LOGITS_FILTER_KWARGS
        request_keys = (self._REQUEST_KEYS | {"length_penalty"} if own_beams else self._REQUEST_KEYS) | {"code_prefix", "audio_format"} | \
            set(_LOGITS_FILTER_KWARGS)
        refuse_code_prefix(gk, "infer_requests(**defaults)")                 # a request key: every segment has its own codes
        inflight_slots, inflight_beam_slots = gk.pop("inflight_slots", None), gk.pop("inflight_beam_slots", None)
        inflight_kw = {k: gk.pop(k) for k in ("chunk_tokens", "min_free") if k in gk}
        base = dict(top_p=gk.pop("top_p", 0.8), top_k=gk.pop("top_k", 30), temperature=gk.pop("temperature", 0.8),
                    repetition_penalty=gk.pop("repetition_penalty", 10.0), max_mel_tokens=gk.pop("max_mel_tokens", 1500), seed=gk.pop("seed", None),
                    typical_sampling=gk.pop("typical_sampling", False), typical_mass=gk.pop("typical_mass", 0.9),
                    best_of=self._best_of(gk.pop("best_of", None), "infer_requests"))
        # "rescore": the numbers come from ONE teacher-forced pass over the chosen codes after decoding (`UnifiedVoice.rescore`), under any
        # num_beams / beam settings / in-flight slots; True keeps its meaning (the decode step's own export, num_beams = 1) and its refusals
        rescore_scores, rescore_ts = self._rescore_flag(gk, "token_scores"), self._rescore_flag(gk, "timestamps")
        want_scores = bool(gk.pop("token_scores", False))
        self.last_scores = None
        timestamps = bool(gk.pop("timestamps", False))
        heads = gk.pop("alignment_heads", None)
        self.last_timestamps = None
        if rescore_ts:
            heads = heads if heads is not None else getattr(self, "alignment_heads", None)
            if heads is None:
                raise ValueError("infer_requests: timestamps='rescore' needs alignment_heads=[(layer, head), ...] (the kwarg, or the attribute "
                                 "`alignment_heads`): no default list is shipped -- rank a checkpoint's heads with TokenAlignment.monotonicity")
            from .gpt import alignment_pairs
            heads = alignment_pairs(heads, int(self.gpt.layers), int(self.gpt.heads), "infer_requests")
        elif timestamps:
            if num_beams != 1:
                raise ValueError(f"infer_requests: timestamps=True applies to num_beams = 1 only (got num_beams = {num_beams}): the text "
                                 "attention of a beam's rows is not exported")
            heads = heads if heads is not None else getattr(self, "alignment_heads", None)
            if heads is None:
                raise ValueError("infer_requests: timestamps=True needs alignment_heads=[(layer, head), ...] (the kwarg, or the attribute "
                                 "`alignment_heads`): no default list is shipped -- rank a checkpoint's heads with TokenAlignment.monotonicity")
            from .gpt import alignment_pairs
            heads = alignment_pairs(heads, int(self.gpt.layers), int(self.gpt.heads), "infer_requests")
        elif heads is not None:
            raise ValueError("infer_requests: alignment_heads is given without timestamps=True")
        # ---- per request: bundle, emotion vector, segments, settings ----
        bundles, bundle_of = [], {}
        latents = {}                                       # (bundle, emotion settings) -> conditioning latents (1, 3, D)
        rows_text, rows_lang, rows_req, rows_seg, rows_bundle, rows_lat = [], [], [], [], [], []
        settings = []
        capacity = self.gpt.n_text_pos
        s2_rows = []                                       # the normalised settings of every request
        for r, req in enumerate(requests):                 # every request's settings are checked before any request costs work
            s2_rows.append(self._request_settings(r, req, request_keys, s2_base, base))
        if num_beams != 1 and any(st["best_of"] > 1 for st in s2_rows):
            raise ValueError(f"infer_requests: `best_of` > 1 applies to num_beams = 1 only (got num_beams = {num_beams}): a beam search already "
                             "keeps its own hypotheses")
        if num_beams != 1 and want_scores:
            raise ValueError("infer_requests: token_scores=True is implemented for num_beams = 1 only")
        # the requests' logits filters over the call's: all equal -> the call-wide path with those values (no table, the launches of a call
        # without request filters); else one entry per row (group) for the engine to merge over the call's kwargs
        req_filters = [self._request_filters(req) for req in requests]
        call_filters = {k: gk[k] for k in _LOGITS_FILTER_KWARGS if k in gk}
        merged_filters = [dict(call_filters, **rf) for rf in req_filters]
        own_filters = any(m != merged_filters[0] for m in merged_filters)
        if not own_filters:
            gk.update(merged_filters[0])
        elif num_beams != 1 and not own_beams:
            differ = sorted(k for k in _LOGITS_FILTER_KWARGS if any(m.get(k) != merged_filters[0].get(k) for m in merged_filters))
            raise ValueError(f"infer_requests: with num_beams = {num_beams} and beam_settings='shared' the requests of a batch must share their "
                             f"logits filters ({differ} differ); pass beam_settings='own' for per-request filters under beam search, or num_beams=1")
        any_prefix = any(req.get("code_prefix") is not None for req in requests)
        if any_prefix and num_beams != 1:
            raise NotImplementedError(f"infer_requests: `code_prefix` is implemented for num_beams = 1 only (got num_beams = {num_beams}): a beam "
                                      "group's rows would share the given codes and their scores")
        if any_prefix and timestamps:
            raise ValueError("infer_requests: timestamps=True with `code_prefix`: the decode export has no rows for given codes; use "
                             "timestamps='rescore', which runs over the full codes")
        if prompt_batching:                                # every cold prompt of the call through ONE prompt-side pass; the loop below then only hits
            self._warm_prompt_caches(requests)
        rows_prefix = []                                   # per row: the segment's given codes, or None
        for r, req in enumerate(requests):
            bi, kl = self._request_conditioning(req, bundles, bundle_of, latents)
            st = s2_rows[r]
            if own_beams:
                st["length_penalty"] = float(req["length_penalty"] if req.get("length_penalty") is not None else length_penalty)
            settings.append(st)
            segs = self.frontend.text_segments(req["text"], req["lang"], max_text_tokens_per_segment, text_normalization, capacity)
            rows_prefix += self._request_prefix(r, req.get("code_prefix"), len(segs))
            for j, seg in enumerate(segs):
                rows_text.append(seg)
                rows_lang.append(self.frontend.lang_id(req["lang"]))
                rows_req.append(r)
                rows_seg.append(j)
                rows_bundle.append(bi)
                rows_lat.append(latents[kl])
        if not rows_text:
            return [None] * len(requests)
        N, dev = len(rows_text), self.device
        L = max(int(t.numel()) for t in rows_text)
        text = torch.full((N, L), 1, dtype=torch.int32)                         # stop_text_token right padding (:726)
        for i, t in enumerate(rows_text):
            text[i, : t.numel()] = t.reshape(-1).to(torch.int32)
        langs = torch.tensor(rows_lang, dtype=torch.long)
        conds = torch.cat(rows_lat, 0)                                         # (N, 3, D): every row under its own voice and emotion
        caps = [int(settings[r]["max_mel_tokens"]) for r in rows_req]
        t0 = time.perf_counter()
        if num_beams == 1:
            for st in settings:                            # one seed per request (drawn like `generate` draws the call's)
                if st["seed"] is None:
                    st["seed"] = self.gpt._seed(None, True, None)
            table = [dict(do_sample=True, top_k=int(settings[r]["top_k"]), top_p=float(settings[r]["top_p"]),
                          temperature=float(settings[r]["temperature"]), repetition_penalty=float(settings[r]["repetition_penalty"]),
                          typical_mass=float(settings[r]["typical_mass"]) if settings[r]["typical_sampling"] else 0.0,
                          stream=j, seed=int(settings[r]["seed"])) for r, j in zip(rows_req, rows_seg)]
            # best_of: row i decodes as its request's `best_of` candidate rows, adjacent; candidate c draws from stream j + (c << 16), so
            # candidate 0 is the row itself and best_of = 1 everywhere leaves the table and the batch as they are
            n_cand = [settings[r]["best_of"] for r in rows_req]
            cand_row = [i for i in range(N) for _ in range(n_cand[i])]
            first_cand = [0] * N
            for i in range(1, N):
                first_cand[i] = first_cand[i - 1] + n_cand[i - 1]
            if len(cand_row) > N:
                if any(n_cand[i] > 1 and rows_seg[i] >= 65536 for i in range(N)):
                    raise ValueError("infer_requests: `best_of` > 1 keys candidate c of segment j by stream j + (c << 16): a request may have at "
                                     "most 65535 segments")
                table = [dict(table[i], stream=rows_seg[i] + ((m - first_cand[i]) << 16)) for m, i in enumerate(cand_row)]
                text_c, langs_c, conds_c, caps_c = text[cand_row], langs[cand_row], conds[cand_row], [caps[i] for i in cand_row]
            else:
                text_c, langs_c, conds_c, caps_c = text, langs, conds, caps
            want_scores = want_scores or len(cand_row) > N
            call = dict(conds_latent=conds_c, do_sample=True, num_beams=1, length_penalty=length_penalty, max_generate_length=max(caps),
                        row_max_new=caps_c, row_sampling=table, **gk)
            if want_scores:
                call["token_scores"] = True
            if timestamps:
                call["alignment_heads"] = heads
            if any_prefix:                                 # every candidate of a row continues the row's given codes; candidate 0 draws from the
                call["code_prefix"] = [rows_prefix[i] for i in cand_row]      # row's own stream: with the original seed it resumes the original
            if own_filters:                                # every segment and every candidate of a request under the request's entry
                call["row_filters"] = [req_filters[rows_req[i]] for i in cand_row]
            if inflight_slots and len(cand_row) > int(inflight_slots):
                codes, _ = self.gpt.inference_speech_inflight(None, text_c.to(dev), langs_c.to(dev), slots=int(inflight_slots), **inflight_kw, **call)
            else:
                codes, _ = self.gpt.inference_speech(None, text_c.to(dev), langs_c.to(dev), **call)
            if want_scores:                                # ---- choose every row's winner; only the winners go on to codes -> mel ----
                ts = self.gpt.last_scores
                means, lens_c, ended_c = ts.mean_logprob().tolist(), ts.lengths.tolist(), ts.ended.tolist()
                report = [[] for _ in requests]
                win = []
                for i in range(N):
                    lo, hi = first_cand[i], first_cand[i] + n_cand[i]
                    chosen = self._choose_candidate(means[lo:hi], ended_c[lo:hi])
                    win.append(lo + chosen)
                    report[rows_req[i]].append(dict(chosen=chosen, mean_logprob=means[lo:hi], lengths=lens_c[lo:hi], ended=ended_c[lo:hi]))
                self.last_scores = report
                if len(cand_row) > N:
                    codes = codes[torch.as_tensor(win, device=codes.device)]
            if timestamps:                                 # the winners' text attention, one row per segment
                al = self.gpt.last_alignment
                al_rows = [al.row(w) for w in (win if len(cand_row) > N else range(N))]
        elif own_beams:
            for st in settings:                            # one seed per request, as above
                if st["seed"] is None:
                    st["seed"] = self.gpt._seed(None, True, None)
            if any(c < 1 for c in caps):
                raise ValueError("infer_requests: max_mel_tokens must be >= 1 (a beam search runs at least its first step)")
            table = [dict(do_sample=True, top_k=int(settings[r]["top_k"]), top_p=float(settings[r]["top_p"]),
                          temperature=float(settings[r]["temperature"]), repetition_penalty=float(settings[r]["repetition_penalty"]),
                          typical_mass=float(settings[r]["typical_mass"]) if settings[r]["typical_sampling"] else 0.0,
                          length_penalty=float(settings[r]["length_penalty"]), stream=j, seed=int(settings[r]["seed"]))
                     for r, j in zip(rows_req, rows_seg)]
            # the call's scalars (range-checked by the engine, otherwise unused while the table is installed): the first request's
            st = settings[0]
            call = dict(conds_latent=conds, do_sample=True, top_p=st["top_p"], top_k=st["top_k"], temperature=st["temperature"],
                        length_penalty=length_penalty, num_beams=num_beams, repetition_penalty=st["repetition_penalty"],
                        max_generate_length=max(caps), row_max_new=caps, group_sampling=table, **gk)
            if own_filters:
                call["group_filters"] = [req_filters[r] for r in rows_req]
            if inflight_beam_slots and N > int(inflight_beam_slots):
                codes, _ = self.gpt.inference_speech_inflight_beams(None, text.to(dev), langs.to(dev), slots=int(inflight_beam_slots),
                                                                    **inflight_kw, **call)
            else:
                codes, _ = self.gpt.inference_speech(None, text.to(dev), langs.to(dev), num_return_sequences=1, **call)
        else:
            differ = [k for k in self._REQUEST_SAMPLING if any(st[k] != settings[0][k] for st in settings)]
            if differ:
                raise ValueError(f"infer_requests: with num_beams = {num_beams} and beam_settings='shared' the requests of a batch must share "
                                 f"their sampling settings ({differ} differ); pass beam_settings='own' for per-request settings under beam "
                                 "search, or num_beams=1")
            st = settings[0]
            call = dict(conds_latent=conds, do_sample=True, top_p=st["top_p"], top_k=st["top_k"], temperature=st["temperature"],
                        length_penalty=length_penalty, num_beams=num_beams, repetition_penalty=st["repetition_penalty"],
                        max_generate_length=st["max_mel_tokens"], typical_sampling=st["typical_sampling"], typical_mass=st["typical_mass"], **gk)
            if st["seed"] is None and keyed_noise:         # the noise is keyed by the call's seed: draw it here, as `generate` would
                st["seed"] = self.gpt._seed(None, True, None)
            if st["seed"] is not None:
                call["seed"] = st["seed"]
            if inflight_beam_slots and N > int(inflight_beam_slots):
                codes, _ = self.gpt.inference_speech_inflight_beams(None, text.to(dev), langs.to(dev), slots=int(inflight_beam_slots),
                                                                    **inflight_kw, **call)
            else:
                codes, _ = self.gpt.inference_speech(None, text.to(dev), langs.to(dev), num_return_sequences=1, **call)
        torch.cuda.synchronize() if torch.cuda.is_available() else None
        t1 = time.perf_counter()
        self.last_codes = codes
        if rescore_scores or rescore_ts:                   # ONE batched teacher-forced pass over the chosen codes of every segment
            from .gpt import TokenScores
            own_lens, _ = TokenScores.lengths_of(codes, caps, int(self.stop_mel_token))
            rs, ra = self.gpt.inference_speech_rescore(None, text.to(dev), codes, langs=langs.to(dev), conds_latent=conds,
                                                       code_lens=own_lens.tolist(), alignment_heads=heads if rescore_ts else None)
            means, lens_r = rs.mean_logprob().tolist(), rs.lengths.tolist()
            if self.last_scores is None:
                self.last_scores = [[] for _ in requests]
                for i in range(N):
                    self.last_scores[rows_req[i]].append(dict(mean_logprob=means[i], lengths=lens_r[i]))
            else:                                          # beside a best_of report (its numbers are the candidates' in-step scores)
                for i in range(N):
                    self.last_scores[rows_req[i]][rows_seg[i]].update(rescored_mean_logprob=means[i], rescored_lengths=lens_r[i])
            if rescore_ts:
                al_rows = [ra.row(i) for i in range(N)]
            torch.cuda.synchronize() if torch.cuda.is_available() else None
            t1 = time.perf_counter()
        codes, code_lens = self.trim_codes(codes)
        hit_cap = [rows_req[i] for i in range(N) if int(code_lens[i]) >= caps[i]]
        if hit_cap:
            warnings.warn(f"WARN: generation stopped due to exceeding `max_mel_tokens` in requests {sorted(set(hit_cap))}. Consider reducing "
                          f"`max_text_tokens_per_segment`({max_text_tokens_per_segment}) or increasing `max_mel_tokens`.", category=RuntimeWarning)
        dur = [float(requests[r].get("duration_factor", 1.0)) for r in rows_req]
        if self.s2mel is not None and self.semantic_codec is not None:
            noise_keys = None
            if keyed_noise:                                # keyed like the row's token draw
                if num_beams == 1 or own_beams:
                    noise_keys = ([int(settings[r]["seed"]) for r in rows_req], list(rows_seg))
                else:
                    noise_keys = ([int(settings[0]["seed"])] * N, list(range(N)))
            s2kw = {}
            for name, key, cast in (("diffusion_steps", "diffusion_steps", int), ("inference_cfg_rate", "inference_cfg_rate", float),
                                    ("noise_temperature", "cfm_temperature", float)):
                col = [cast(settings[r][key]) for r in rows_req]
                s2kw[name] = col if any(v != col[0] for v in col) else col[0]      # one value per row only where the rows differ: one solve otherwise
            mel, mel_lens = self.codes_to_mel(codes, code_lens, bundles, dur, bundle_index=rows_bundle, noise_keys=noise_keys, **s2kw)
        else:                                              # codes -> mel on the frontend's PyTorch modules: one call per voice and duration factor
            groups: Dict[tuple, List[int]] = {}
            for i in range(N):
                groups.setdefault((rows_bundle[i], dur[i]), []).append(i)
            parts = {}
            for (bi, d), idx in groups.items():
                m_g, l_g = self.frontend.codes_to_mel(codes[idx], code_lens[idx], bundles[bi], d)
                for k, i in enumerate(idx):
                    parts[i] = m_g[k, :, : int(l_g[k])]
            mel_lens = torch.tensor([parts[i].shape[-1] for i in range(N)], dtype=torch.int32)
            mel = torch.zeros(N, parts[0].shape[0], int(mel_lens.max()), device=parts[0].device)
            for i in range(N):
                mel[i, :, : parts[i].shape[-1]] = parts[i]
        torch.cuda.synchronize() if torch.cuda.is_available() else None
        t2 = time.perf_counter()
        wav = self.bigvgan(mel.float(), lens=mel_lens)                      # the v2.5 vocoder has no speaker input
        rows_f32 = wav[:, 0, :]                                             # in [-1, 1], on the device: what the delivery formats start from
        up = self.bigvgan.total_up
        row_samples = [int(mel_lens[i]) * up for i in range(N)]
        wavs = [None] * N                                                   # the host rows of the requests without a format, as always
        if any(f is None for f in formats):
            wav = torch.clamp(PCM16_MAX * wav, -PCM16_MAX, PCM16_MAX)
            wavs = [wav[i, :, : row_samples[i]].cpu() if formats[rows_req[i]] is None else None for i in range(N)]
        if timestamps or rescore_ts:
            # code i of a row starts at sample i * 2 * 1.72 * duration_factor * up of its segment (the stretch `codes_to_mel` applies), the
            # segment starts after the request's earlier segments and one silence each
            sil = int(22050 * interval_silence / 1000.0) if interval_silence > 0 else 0
            report, offset = [[] for _ in requests], [0] * len(requests)
            start_t, stop_t = int(self.gpt.start_text_token), int(self.gpt.stop_text_token)
            for i in range(N):
                r, n_codes, samples = rows_req[i], int(code_lens[i]), row_samples[i]
                ids = [int(v) for v in rows_text[i].reshape(-1).tolist() if int(v) not in (start_t, stop_t)]
                spans = al_rows[i].path(0, "mean", n_codes=n_codes)
                report[r].append(self.segment_timestamps(spans, ids, n_codes, samples, 2 * 1.72 * dur[i] * up, offset[r]))
                offset[r] += samples + sil
            self.last_timestamps = report
        t3 = time.perf_counter()
        self.last_timing = dict(gpt=t1 - t0, s2mel=t2 - t1, bigvgan=t3 - t2)
        out = []
        for r in range(len(requests)):
            seg = [w for w, o in zip(wavs, rows_req) if o == r]
            if not seg or formats[r] is not None:
                out.append(None)
                continue
            w = torch.cat(self.insert_interval_silence(seg, 22050, interval_silence), dim=1)
            out.append((22050, w.type(torch.int16).numpy().T))
        by_format: Dict[object, List[int]] = {}
        for r, f in enumerate(formats):
            if f is not None and r in rows_req:
                by_format.setdefault(f, []).append(r)
        loudness, limiter = [None] * len(requests), [None] * len(requests)
        for f, reqs in by_format.items():                  # one conversion and one device-to-host copy per format of the call
            from . import output
            groups = [[i for i in range(N) if rows_req[i] == r] for r in reqs]
            measured, limited = [], []
            arrays = output.convert(rows_f32, row_samples, groups, f, interval_silence, report=measured, limiter_report=limited)
            for r, a, m, lim in zip(reqs, arrays, measured, limited):
                out[r] = (f.sample_rate, a.reshape(-1, 1))
                loudness[r], limiter[r] = m, lim
        self.last_loudness, self.last_limiter = loudness, limiter
        return out

    # ---- streaming sessions: streams arrive one at a time, each with its own voice ------------------------------------------------------
    def stream_session(self, slots, chunk_size: int = 100, overlap_size: int = 20, max_mel_tokens: int = 1500, max_text_tokens_per_segment=120,
                       poll_steps: int = 8, text_normalization=True, cfm_noise="request", **defaults):
        """An open-ended `infer_stream`: -> `streaming.StreamSession` over `slots` decode slots.  `submit(request)` takes the dict
        `infer_requests` takes (same keys, same checks; one text of one segment) and returns a stream id; the stream starts as soon as a decode
        slot is free (FIFO while none is).  `step()` advances the decode session by at most `poll_steps` steps, refills freed slots and renders
        every chunk that became due -- rows at different chunk indices and of different voices -- in ONE codes -> mel call and ONE ragged vocoder
        call; it returns events `(stream id, 22050, int16 array or None, done, chunk index)`.  `events()` iterates `step()`, `cancel(id)` stops a
        stream, `close()` releases the engine (until then every other generate call on this object is refused, as during `infer_stream`).
        `**defaults`: sampling and codes -> mel defaults as in `infer_requests`; `num_beams` is forced to 1 as in `infer_stream`;
        `max_mel_tokens` is the session's bound on a stream's codes and the default cap of a request.

        The invariant: with `cfm_noise="request"` (the default; needs the engine's codec / s2mel stages) a stream's events -- pieces, done flags,
        chunk indices -- are bit for bit what `infer_stream(voice, [text], lang, seed=<its seed>, max_mel_tokens=<its cap>, chunk_size=...,
        overlap_size=..., cfm_noise="request", <its settings>)` yields for its one row, whatever slot it got, whatever step it joined at, whatever
        its batch mates are and whatever `poll_steps` is (which only delays a chunk to the next poll).  With `cfm_noise="global"` the flow-matching
        noise comes from torch's generator, one draw per render call, and only the CODES of a stream are invariant.  A request without a seed
        draws one from torch's generator at submit.

        `audio_format` (a session default in `**defaults`, and a request key that wins over it): the stream's pieces are made on the device --
        cross-fade, streaming resampler, encoding: one launch each per render for all its jobs, one device-to-host copy per format
        (`output.deliver`) -- and its events carry the format's rate and dtype.  The pieces of a stream concatenate to the bits of the one-shot
        conversion of its 22050 Hz pieces, and are those of `infer_stream(..., audio_format=<its format>)` of the request alone; streams of
        different formats, and streams without one, share a session.  `peak_dbfs` needs the whole request: refused at submit."""
        from . import dist as D
        from .streaming import StreamSession
        self._audio_format(defaults.get("audio_format"), "stream_session")      # refused before anything else where it cannot run
        if D.world() > 1:
            raise NotImplementedError("stream_session under torch.distributed: the decode session lives on one device (use infer_batch)")
        if self.SPK_COND_MODE != "campplus":
            raise NotImplementedError("stream_session is implemented for the IndexTTS-2.5 pipeline (campplus conditioning)")
        backend = _StreamBackend(self, int(slots), int(max_mel_tokens), max_text_tokens_per_segment, text_normalization, cfm_noise, defaults)
        return StreamSession(backend, slots, chunk_size=chunk_size, overlap_size=overlap_size, poll_steps=poll_steps)

    # ---- the hot path: one GPT batch, one ragged vocoder batch -------------------------------------------------------
    def _synthesize(self, segment_tokens: List[torch.Tensor], lang_ids: List[int], bundle, emovec, duration_factor,
                    generation_kwargs, max_text_tokens_per_segment, device_rows: bool = False) -> List[torch.Tensor]:
        """-> per segment its PCM-scale (+-32767) waveform (1, T) on the host; `device_rows`: -> (rows (B, T) on the device in [-1, 1], their
        lengths) for `output.convert` instead -- no per-row copy"""
        gk = dict(generation_kwargs)
        from .gpt import refuse_code_prefix
        refuse_code_prefix(gk, "infer / infer_batch")
        gk.pop("do_sample", None)                       # popped and ignored by the reference too (:732,781)
        top_p, top_k = gk.pop("top_p", 0.8), gk.pop("top_k", 30)
        temperature = gk.pop("temperature", 0.8)
        length_penalty = gk.pop("length_penalty", 0.0)
        num_beams = gk.pop("num_beams", 3)
        repetition_penalty = gk.pop("repetition_penalty", 10.0)
        max_mel_tokens = gk.pop("max_mel_tokens", 1500)
        dev = self.device
        L = max(int(t.numel()) for t in segment_tokens)
        text = torch.full((len(segment_tokens), L), 1, dtype=torch.int32)      # stop_text_token right padding (:726)
        for i, t in enumerate(segment_tokens):
            text[i, : t.numel()] = t.reshape(-1).to(torch.int32)
        langs = torch.tensor(lang_ids, dtype=torch.long)
        inflight_slots = gk.pop("inflight_slots", None)    # engine extension: decode `inflight_slots` rows at a time, admit waiting segments into
        inflight_beam_slots = gk.pop("inflight_beam_slots", None)    # the same for num_beams > 1: that many beam GROUPS search at a time (explicit:
                                                                     # `inflight_slots` with beams stays the plain batch call)
        inflight_kw = {k: gk.pop(k) for k in ("chunk_tokens", "min_free") if k in gk}              # slots whose row has stopped
        s2kw = {}
        if self._cfm_noise_mode(gk) == "request":          # (popped here: it never reaches inference_speech) noise of row i keyed by (seed, i)
            self._need_engine_s2mel("cfm_noise='request'")
            if gk.get("seed") is None:
                gk["seed"] = self.gpt._seed(None, True, None)
            s2kw["noise_keys"] = ([int(gk["seed"])] * len(segment_tokens), list(range(len(segment_tokens))))
        t0 = time.perf_counter()
        if inflight_slots and num_beams == 1 and len(segment_tokens) > int(inflight_slots):
            codes, _ = self.gpt.inference_speech_inflight(bundle["spk_cond_emb"], text.to(dev), langs.to(dev), emo_vec=emovec,
                                                          campplus_embedding=bundle["style"], do_sample=True, top_p=top_p, top_k=top_k,
                                                          temperature=temperature, length_penalty=length_penalty, num_beams=1,
                                                          repetition_penalty=repetition_penalty, max_generate_length=max_mel_tokens,
                                                          slots=int(inflight_slots), **inflight_kw, **gk)
        elif inflight_beam_slots and num_beams > 1 and len(segment_tokens) > int(inflight_beam_slots):
            codes, _ = self.gpt.inference_speech_inflight_beams(bundle["spk_cond_emb"], text.to(dev), langs.to(dev), emo_vec=emovec,
                                                                campplus_embedding=bundle["style"], do_sample=True, top_p=top_p, top_k=top_k,
                                                                temperature=temperature, length_penalty=length_penalty, num_beams=num_beams,
                                                                repetition_penalty=repetition_penalty, max_generate_length=max_mel_tokens,
                                                                slots=int(inflight_beam_slots), **inflight_kw, **gk)
        else:
            codes, _ = self.gpt.inference_speech(bundle["spk_cond_emb"], text.to(dev), langs.to(dev), emo_vec=emovec,
                                                 campplus_embedding=bundle["style"], do_sample=True, top_p=top_p, top_k=top_k,
                                                 temperature=temperature, num_return_sequences=1, length_penalty=length_penalty,
                                                 num_beams=num_beams, repetition_penalty=repetition_penalty,
                                                 max_generate_length=max_mel_tokens, **gk)
        torch.cuda.synchronize() if torch.cuda.is_available() else None
        t1 = time.perf_counter()
        if codes.shape[1] > 0 and (codes[:, -1] != self.stop_mel_token).any():
            warnings.warn(f"WARN: generation stopped due to exceeding `max_mel_tokens` ({max_mel_tokens}). "
                          f"Consider reducing `max_text_tokens_per_segment`({max_text_tokens_per_segment}) or increasing "
                          f"`max_mel_tokens`.", category=RuntimeWarning)
        codes, code_lens = self.trim_codes(codes)
        if self.s2mel is not None and self.semantic_codec is not None:
            mel, mel_lens = self.codes_to_mel(codes, code_lens, bundle, duration_factor, **s2kw)
        else:
            mel, mel_lens = self.frontend.codes_to_mel(codes, code_lens, bundle, duration_factor)
        torch.cuda.synchronize() if torch.cuda.is_available() else None
        t2 = time.perf_counter()
        wav = self.bigvgan(mel.float(), lens=mel_lens)                      # (B, 1, Tmax*256), rows bounded at own length
        up = self.bigvgan.total_up
        if device_rows:
            torch.cuda.synchronize() if torch.cuda.is_available() else None
            self.last_timing = dict(gpt=t1 - t0, s2mel=t2 - t1, bigvgan=time.perf_counter() - t2)
            return wav[:, 0, :], [int(n) * up for n in mel_lens]
        wav = torch.clamp(PCM16_MAX * wav, -PCM16_MAX, PCM16_MAX)           # (:855)
        out = [wav[i, :, : int(mel_lens[i]) * up].cpu() for i in range(wav.shape[0])]
        t3 = time.perf_counter()
        self.last_timing = dict(gpt=t1 - t0, s2mel=t2 - t1, bigvgan=t3 - t2)
        return out


W2V_TAP_LAYER = 17                    # `hidden_states[17]` of the w2v-bert-2.0 encoder (infer_v2_5.py:288)


class _StreamItem:
    """a submitted stream as the engine needs it"""
    __slots__ = ("text", "lang_id", "latent", "bundle", "entry", "cap", "seed", "dur", "s2", "filters", "audio_format")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class _StreamBackend:
    """What `streaming.StreamSession` asks of the engine (its docstring lists the methods), for the IndexTTS-2.5 pipeline: one
    `gpt.DecodeSession` with a per-slot sampling table and per-slot caps, opened lazily over the first batch.  Capacity: a `DecodeSession` sizes
    its cache rows from the first batch, so that batch's prompts are left-padded to the longest text `max_text_tokens_per_segment` admits, and
    slots without a stream start with a row whose cap is 0 (it ends at step 0 and is admittable) -- a session opened by one short request then
    admits any prompt, and runs with fewer streams than slots."""

    def __init__(self, tts: "IndexTTS2", slots: int, max_mel_tokens: int, max_text_tokens_per_segment, text_normalization, cfm_noise, defaults):
        self.tts, self.slots, self.max_new = tts, slots, int(max_mel_tokens)
        self.max_text, self.text_normalization = int(max_text_tokens_per_segment), text_normalization
        gk = dict(defaults)
        from .output import stream_format
        self.audio_format = stream_format(tts._audio_format(gk.pop("audio_format", None), "stream_session"), "stream_session")
        gk["cfm_noise"] = cfm_noise
        self.keyed = tts._cfm_noise_mode(gk) == "request"
        if self.keyed:
            tts._need_engine_s2mel("cfm_noise='request'")
        gk.pop("do_sample", None)
        gk.pop("num_beams", None)                          # one hypothesis per row, as infer_stream
        tts._refuse_timestamps(gk, "stream_session")
        from .gpt import refuse_code_prefix
        refuse_code_prefix(gk, "stream_session")
        if tts._best_of(gk.pop("best_of", None), "stream_session") > 1:
            raise ValueError("stream_session: `best_of` > 1 is not available to streams (a stream's codes leave before its row ends)")
        self.s2_base = {k: gk.pop(k, None) for k in tts._REQUEST_S2MEL}
        self.length_penalty = gk.pop("length_penalty", 0.0)
        self.base = dict(top_p=gk.pop("top_p", 0.8), top_k=gk.pop("top_k", 30), temperature=gk.pop("temperature", 0.8),
                         repetition_penalty=gk.pop("repetition_penalty", 10.0), max_mel_tokens=self.max_new, seed=gk.pop("seed", None),
                         typical_sampling=gk.pop("typical_sampling", False), typical_mass=gk.pop("typical_mass", 0.9))
        self.gk = gk                                       # what is left goes to the decode session, as infer_stream hands it to generate
        # text ids of a segment: at most max_text_tokens_per_segment tokens, the language tag and the stop id; never more than the text
        # position table holds between its start and stop rows
        self.text_width = max(1, min(self.max_text + 2, int(tts.gpt.n_text_pos) - 2))
        self.bundles, self.bundle_of, self.latents = [], {}, {}
        self.sess = None
        self.n_submitted = 0

    @property
    def steps(self) -> int:
        return 0 if self.sess is None else self.sess.steps

    def frames_per_code(self, item) -> float:
        return 2 * 1.72 * item.dur                         # int(2 * n * 1.72 * duration_factor) frames for n codes, as infer_stream

    def prepare(self, req: dict) -> _StreamItem:
        tts, r = self.tts, self.n_submitted
        from .gpt import _LOGITS_FILTER_KWARGS
        st = tts._request_settings(r, req, tts._REQUEST_KEYS | {"audio_format"} | set(_LOGITS_FILTER_KWARGS), self.s2_base, self.base)
        from .output import stream_format
        fmt = stream_format(tts._audio_format(req.get("audio_format"), f"request {r}"), f"request {r}") or self.audio_format
        if st["best_of"] > 1:                              # candidates are compared when their rows have ended; a stream's codes leave before that
            raise ValueError(f"request {r}: `best_of` = {st['best_of']} is not available to streams (a stream's codes leave before its row "
                             "ends); use infer_requests")
        cap = int(st["max_mel_tokens"])
        if not 0 <= cap <= self.max_new:
            raise ValueError(f"request {r}: max_mel_tokens = {cap} is outside the session's 0 .. {self.max_new}")
        segs = tts.frontend.text_segments(req["text"], req["lang"], self.max_text, self.text_normalization, tts.gpt.n_text_pos)
        if len(segs) != 1:
            raise ValueError(f"request {r}: a stream takes a text of one segment, got {len(segs)} (split long texts with the frontend first)")
        text = segs[0].reshape(-1).to(torch.int32)
        if text.numel() > self.text_width:
            raise ValueError(f"request {r}: the segment has {text.numel()} text ids, the session's prompts hold {self.text_width}")
        if len(self.latents) >= 64:                        # the prompt encoders' results stay in the pipeline's LRUs
            self.bundles, self.bundle_of, self.latents = [], {}, {}
        bi, kl = tts._request_conditioning(req, self.bundles, self.bundle_of, self.latents)
        # the request's filters are checked HERE, against its own cap and its own prompt (the shortest it can be admitted with: a wider
        # admission batch only relaxes min_length), so a bad value goes to the submitting caller and never to the session's other streams
        filters = tts._request_filters(req)
        from .gpt import row_filter_entries
        stop = int(tts.stop_mel_token)
        try:
            row_filter_entries([filters], 1, self.gk, int(getattr(tts.gpt, "number_mel_codes", stop + 1)), stop, self.max_new, 1, "stream_session",
                               prompt_len=int(self.latents[kl].shape[1]) + int(text.numel()) + 3, row_max_new=[cap], name="filters")
        except (ValueError, NotImplementedError) as e:
            raise type(e)(f"request {r}: {e}") from e
        seed = int(st["seed"]) if st["seed"] is not None else tts.gpt._seed(None, True, None)
        entry = dict(do_sample=True, top_k=int(st["top_k"]), top_p=float(st["top_p"]), temperature=float(st["temperature"]),
                     repetition_penalty=float(st["repetition_penalty"]),
                     typical_mass=float(st["typical_mass"]) if st["typical_sampling"] else 0.0, stream=0, seed=seed)
        self.n_submitted += 1
        return _StreamItem(text=text, lang_id=tts.frontend.lang_id(req["lang"]), latent=self.latents[kl], bundle=self.bundles[bi], entry=entry,
                           cap=cap, seed=seed, dur=float(req.get("duration_factor", 1.0)),
                           s2={k: st[k] for k in tts._REQUEST_S2MEL}, filters=filters, audio_format=fmt)

    def _prompts(self, items, width: int):
        dev = self.tts.device
        text = torch.full((len(items), width), 1, dtype=torch.int32)                # stop_text_token right padding, left-padded by the engine
        for i, it in enumerate(items):
            text[i, : it.text.numel()] = it.text
        langs = torch.tensor([it.lang_id for it in items], dtype=torch.long)
        return text.to(dev), langs.to(dev), torch.cat([it.latent for it in items], 0)

    def open(self, items):
        from .gpt import DecodeSession
        gpt = self.tts.gpt
        table = int(gpt._emb["mel_pos_embedding.emb.weight"].shape[0]) + 1 - (2 if gpt.kv_cache else 1)      # the engine's bound on a ROW's steps
        if self.max_new > table:
            raise ValueError(f"stream_session: max_mel_tokens = {self.max_new} exceeds the mel position table ({table} steps)")
        real = next(it for it in items if it is not None)
        rows = [it if it is not None else real for it in items]                     # an empty slot: any prompt, cap 0
        text, langs, conds = self._prompts(rows, self.text_width)
        emb, mask, max_new, hf, _ = gpt._prepare_inference(None, text, langs, None, None, None, None, 1, self.max_new, False, 0.9, conds,
                                                           dict(self.gk))
        b = self.base
        from .gpt import _LOGITS_FILTER_KWARGS
        off = dict.fromkeys(_LOGITS_FILTER_KWARGS)         # an empty slot: every filter at HF's default, whatever the session's are (its cap is 0)
        self.sess = DecodeSession(gpt, emb, mask, max_new, do_sample=True, top_p=b["top_p"], top_k=b["top_k"], temperature=b["temperature"],
                                  repetition_penalty=b["repetition_penalty"], length_penalty=self.length_penalty, seed=0,
                                  row_max_new=[it.cap if it is not None else 0 for it in items], row_sampling=[it.entry for it in rows],
                                  row_filters=[it.filters if it is not None else off for it in items], **hf)

    def admit(self, slots, items):
        text, langs, conds = self._prompts(items, max(int(it.text.numel()) for it in items))
        _, emb, mask = self.tts.gpt.prepare_gpt_inputs(conds, text, langs)
        self.sess.admit(slots, emb, mask, row_max_new=[it.cap for it in items], row_sampling=[it.entry for it in items],
                        row_filters=[it.filters for it in items])

    def run(self, n: int, return_when_finished: int):
        before = self.sess.steps
        self.sess.run(n, return_when_finished=return_when_finished)
        if self.sess.steps == before:
            from ._lib import HipEngineError
            raise HipEngineError("stream_session: the decode session made no progress")

    def progress(self):
        return self.sess.progress()

    def stop(self, slot: int):
        self.sess.stop_row(slot)

    def collect(self, jobs):
        """the jobs' code windows (R, widest) out of the session's code rows, zero past a window's end, and their lengths"""
        dev, codes = self.tts.device, self.sess._codes
        n = torch.tensor([j[4] for j in jobs], device=dev)
        col = torch.arange(int(n.max()), device=dev)[None, :]
        at = (torch.tensor([j[3] for j in jobs], device=dev)[:, None] + col).clamp(max=codes.shape[1] - 1)
        win = codes[torch.tensor([j[1] for j in jobs], device=dev)[:, None], at]
        return torch.where(col < n[:, None], win, torch.zeros_like(win)), n.to(torch.int32).cpu()

    def render(self, jobs, windows):
        tts = self.tts
        codes, lens = windows
        items = [j[0] for j in jobs]
        R = len(jobs)
        bundles, index = [], []
        for it in items:                                   # the distinct voices of this render, in order of appearance
            hit = [i for i, b in enumerate(bundles) if b is it.bundle]
            if not hit:
                bundles.append(it.bundle)
            index.append(hit[0] if hit else len(bundles) - 1)
        dur = [it.dur for it in items]
        if tts.s2mel is not None and tts.semantic_codec is not None:
            s2kw = {}
            if self.keyed:                                 # (seed, stream 0, chunk): the key infer_stream gives the request alone
                s2kw["noise_keys"] = ([it.seed for it in items], [0] * R, [j[2] for j in jobs])
            for name, key, cast in (("diffusion_steps", "diffusion_steps", int), ("inference_cfg_rate", "inference_cfg_rate", float),
                                    ("noise_temperature", "cfm_temperature", float)):
                col = [cast(it.s2[key]) for it in items]
                s2kw[name] = col if any(v != col[0] for v in col) else col[0]
            mel, mel_lens = tts.codes_to_mel(codes, lens, bundles, dur, bundle_index=index, **s2kw)
        else:                                              # the frontend's PyTorch codes -> mel: one call per voice and duration factor
            groups: Dict[tuple, List[int]] = {}
            for i in range(R):
                groups.setdefault((index[i], dur[i]), []).append(i)
            parts = {}
            for (bi, d), idx in groups.items():
                m_g, l_g = tts.frontend.codes_to_mel(codes[idx], lens[idx], bundles[bi], d)
                for k, i in enumerate(idx):
                    parts[i] = m_g[k, :, : int(l_g[k])]
            mel_lens = torch.tensor([parts[i].shape[-1] for i in range(R)], dtype=torch.int32)
            mel = torch.zeros(R, parts[0].shape[0], int(mel_lens.max()), device=parts[0].device)
            for i in range(R):
                mel[i, :, : parts[i].shape[-1]] = parts[i]
        wav = tts.bigvgan(mel.float(), lens=mel_lens)
        up = tts.bigvgan.total_up
        # a stream with an `audio_format` gets its row as it lies on the device (`StreamSession._deliver` makes the piece there); the others
        # the host array they always got
        return [wav[i, 0, : int(mel_lens[i]) * up].float() if it.audio_format is not None else
                wav[i, 0, : int(mel_lens[i]) * up].float().cpu().numpy() for i, it in enumerate(items)]

    def close(self):
        if self.sess is not None:
            self.sess.close()
            self.sess = None


class ReferenceFrontend(Frontend):
    """Prompt / text stages on the reference's own PyTorch modules.

    The reference package builds every prompt-side module in one place, `indextts.infer_v2_5.IndexTTS2.__init__`
    (:117-266: w2v-bert feature extractor + model + statistics, semantic codec, s2mel, CAMPPlus, tokenizer, text normaliser,
    emotion / speaker matrices, mel function).  Instead of restating that loader, this frontend constructs the reference
    object itself from the same `cfg_path` / `model_dir` (`ref=` injects an existing one) and drives its modules with the call
    sequences of `infer_generator` (:620-727).  The reference's GPT transformer stack and vocoder are not used (the engine
    replaces them) and are dropped after construction; its emotion encoder (`gpt.merge_emovec`) is kept.

    Needs the reference `indextts` package with its third-party dependencies (torchaudio, librosa, transformers, ...) and the
    checkpoint directory: where those are missing the constructor raises ImportError / FileNotFoundError -- there is no fallback.
    """

    def __init__(self, cfg, model_dir, device, gpt_engine=None, cfg_path=None, ref=None):
        if ref is None:
            try:
                from indextts.infer_v2_5 import IndexTTS2 as RefIndexTTS2
            except Exception as e:                                   # loud: there is no fallback
                raise ImportError("ReferenceFrontend needs the reference `indextts` package and its prompt-side dependencies "
                                  f"(torchaudio, librosa, transformers, ...): {e!r}.  Inject frontend= instead, e.g. "
                                  "indextts_amd.frontend.EngineFrontend(cfg, model_dir, device, text_frontend=...), which reads the "
                                  "checkpoint directory itself and needs no reference package.") from e
            ref = RefIndexTTS2(cfg_path=cfg_path or os.path.join(model_dir, "config.yaml"), model_dir=model_dir, use_bf16=False,
                               device=device, use_cuda_kernel=False)
            for name in ("bigvgan",):                                # replaced by the engine
                if hasattr(ref, name):
                    setattr(ref, name, None)
            if getattr(ref, "gpt", None) is not None:
                for name in ("gpt", "inference_model"):              # the GPT-2 stack; merge_emovec / get_emovec stay
                    if hasattr(ref.gpt, name):
                        setattr(ref.gpt, name, None)
        self.ref = ref
        self.cfg, self.model_dir, self.device = cfg, model_dir, device
        self.tokenizer = ref.tokenizer
        # the CAMPPlus speaker encoder runs on the engine (indextts_amd/campplus.py) from the weights the reference module loaded;
        # the reference's own module stays in place only when its configuration is not the shipped one
        self.campplus = None
        cm = getattr(ref, "campplus_model", None)
        if cm is not None and hasattr(cm, "state_dict") and torch.cuda.is_available() and str(device).startswith("cuda"):
            try:
                from .campplus import CAMPPlus
                self.campplus = CAMPPlus(feat_dim=80, embedding_size=192, device=device).load_state_dict(cm.state_dict())
            except NotImplementedError:
                self.campplus = None

        # likewise the w2v-bert-2.0 feature encoder (indextts_amd/w2vbert.py): only the 17 layers below the tapped hidden state
        self.w2v = None
        sm = getattr(ref, "semantic_model", None)
        if sm is not None and hasattr(sm, "config") and torch.cuda.is_available() and str(device).startswith("cuda"):
            try:
                from .w2vbert import Wav2Vec2BertModel
                c = sm.config
                self.w2v = Wav2Vec2BertModel(
                    hidden_size=c.hidden_size, num_hidden_layers=c.num_hidden_layers, num_attention_heads=c.num_attention_heads,
                    intermediate_size=c.intermediate_size, feature_projection_input_dim=c.feature_projection_input_dim,
                    position_embeddings_type=c.position_embeddings_type, left_max_position_embeddings=c.left_max_position_embeddings,
                    right_max_position_embeddings=c.right_max_position_embeddings, conv_depthwise_kernel_size=c.conv_depthwise_kernel_size,
                    hidden_act=c.hidden_act, layer_norm_eps=c.layer_norm_eps, add_adapter=c.add_adapter, device=device,
                ).load_state_dict(sm.state_dict(), n_layers=W2V_TAP_LAYER)
            except NotImplementedError:
                self.w2v = None

        # and the DSP in front of them (indextts_amd/audio.py: resampling, SeamlessM4T features, prompt log-mel, Kaldi fbank): the engine
        # versions take over when the s2mel spectrogram parameters are the ones the kernel supports (win_length == n_fft, center=False)
        self.audio = None
        if torch.cuda.is_available() and str(device).startswith("cuda"):
            try:
                from . import audio as A
                sp = cfg["s2mel"]["preprocess_params"]
                spect = sp["spect_params"]
                fmax = spect.get("fmax", "None") if hasattr(spect, "get") else "None"
                self._mel_args = dict(n_fft=int(spect["n_fft"]), win_size=int(spect["win_length"]), hop_size=int(spect["hop_length"]),
                                      num_mels=int(spect["n_mels"]), sampling_rate=int(sp["sr"]),
                                      fmin=spect.get("fmin", 0) if hasattr(spect, "get") else 0,
                                      fmax=None if fmax == "None" else 8000, center=False)          # infer_v2_5.py:256-265
                if self._mel_args["win_size"] == self._mel_args["n_fft"]:
                    self.audio = A
                    self._features = A.SeamlessM4TFeatureExtractor(device=device)
            except (KeyError, TypeError, AttributeError):
                self.audio = None

    # ---- the reference's own state dicts, for the engine stages (IndexTTS2.__init__ loads them when none are injected) --------
    def engine_state_dicts(self):
        return dict(semantic_codec=self.ref.semantic_codec.state_dict(), cfm=self.ref.s2mel.models["cfm"].state_dict(),
                    length_regulator=self.ref.s2mel.models["length_regulator"].state_dict())

    # ---- infer_generator :620-667 -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _w2v(self, audio_16k):
        r = self.ref
        inputs = (self._features if self.audio is not None else r.extract_features)(audio_16k, sampling_rate=16000, return_tensors="pt")
        if self.w2v is not None:
            return self.w2v.get_emb(inputs["input_features"], inputs["attention_mask"], r.semantic_mean, r.semantic_std, layer=W2V_TAP_LAYER)
        return r.get_emb(inputs["input_features"].to(self.device), inputs["attention_mask"].to(self.device))

    @torch.no_grad()
    def speaker_bundle(self, spk_audio_prompt):
        r = self.ref
        audio, sr = r._load_and_cut_audio(spk_audio_prompt, 15, False)
        if self.audio is not None:                                   # DSP on the engine (indextts_amd/audio.py)
            A = self.audio
            audio_22k = A.Resample(sr, 22050, device=self.device)(audio)
            audio_16k = A.Resample(sr, 16000, device=self.device)(audio)
            spk_cond_emb = self._w2v(audio_16k)
            ref_mel = A.mel_spectrogram(audio_22k, **self._mel_args)
            feat = A.subtract_mean(A.fbank(audio_16k, num_mel_bins=80, dither=0, sample_frequency=16000))
        else:
            import torchaudio
            audio_22k = torchaudio.transforms.Resample(sr, 22050)(audio)
            audio_16k = torchaudio.transforms.Resample(sr, 16000)(audio)
            spk_cond_emb = self._w2v(audio_16k)
            ref_mel = r.mel_fn(audio_22k.to(spk_cond_emb.device).float())
            feat = torchaudio.compliance.kaldi.fbank(audio_16k.to(ref_mel.device), num_mel_bins=80, dither=0, sample_frequency=16000)
            feat = feat - feat.mean(dim=0, keepdim=True)
        style = (self.campplus or r.campplus_model)(feat.unsqueeze(0))
        prompt_condition = r.s2mel.models["length_regulator"](spk_cond_emb, ylens=torch.LongTensor([ref_mel.size(2)]).to(ref_mel.device),
                                                              n_quantizers=3, f0=None)[0]
        return dict(style=style, spk_cond_emb=spk_cond_emb, ref_mel=ref_mel, prompt_condition=prompt_condition)

    @torch.no_grad()
    def emo_cond(self, emo_audio_prompt):                            # :682-697
        emo_audio, _ = self.ref._load_and_cut_audio(emo_audio_prompt, 15, False, sr=16000)
        return self._w2v(emo_audio)

    @torch.no_grad()
    def merge_emovec(self, spk_cond_emb, emo_cond_emb, alpha):       # :759-765 (the lengths are the feature dims there)
        dev = spk_cond_emb.device
        return self.ref.gpt.merge_emovec(spk_cond_emb, emo_cond_emb, torch.tensor([spk_cond_emb.shape[-1]], device=dev),
                                         torch.tensor([emo_cond_emb.shape[-1]], device=dev), alpha=alpha)

    def emo_vector_mix(self, emo_vector, style, use_random):         # :669-680
        import random
        r = self.ref
        from indextts.infer_v2_5 import find_most_similar_cosine
        w = torch.tensor(emo_vector, device=self.device)
        idx = [random.randint(0, x - 1) for x in r.emo_num] if use_random else [find_most_similar_cosine(style, t) for t in r.spk_matrix]
        mat = torch.cat([t[i].unsqueeze(0) for i, t in zip(idx, r.emo_matrix)], 0)
        return torch.sum(w.unsqueeze(1) * mat, 0).unsqueeze(0), torch.sum(w)

    def text_segments(self, text, lang, max_text_tokens_per_segment, text_normalization, capacity):     # :699-726
        import re
        from indextts import infer_v2_5 as R
        r, lo = self.ref, lang.lower()
        prefix = f"<|{lo}|> "
        text = r.text_process.clean_pattern.sub(lambda x: r.text_process.char_rep_map[x.group()], text)
        if text_normalization:
            if lo in ("zh", "zhen", "en"):
                text = r.text_process.normalize(text)
            elif lo in ("ja", "es"):
                text = R.nemo_text_normalize(text, lo)
        if lo in ("ja", "zh", "zhen", "en"):
            text = text.lower()
        if lo == "es":
            text = text.upper()
        text = R.apply_pronunciation_annotations(text)
        if lo == "ja":
            text = r.ja_text_process.process_ja_text(text)
        text = re.sub(r"<\|([^|]+)\|>", lambda m: f"<|{m.group(1).upper()}|>", text)
        out = []
        for seg in r.split_text_by_tokens(text, max_text_tokens_per_segment, prefix):
            toks = r.tokenizer.encode(prefix + seg, allowed_special="all")
            out.append(torch.tensor(list(toks) + [1], dtype=torch.int32))          # F.pad(toks, (0, 1), value=1)
        return out

    def lang_id(self, lang):
        from indextts.utils.tokenizer import lang_to_token
        return int(lang_to_token(lang))

    @torch.no_grad()
    def codes_to_mel(self, codes, code_lens, bundle, duration_factor):            # :830-846, segment by segment at batch 1
        r = self.ref
        mels, lens = [], []
        for b in range(codes.shape[0]):
            n = int(code_lens[b])
            S_infer = r.semantic_codec.decode(codes[b:b + 1, :n])
            target = torch.LongTensor([int(S_infer.shape[1] * 1.72 * duration_factor)]).to(codes.device)
            cond = r.s2mel.models["length_regulator"](S_infer, ylens=target, n_quantizers=3, f0=None)[0]
            cat = torch.cat([bundle["prompt_condition"], cond], dim=1)
            mel = r.s2mel.models["cfm"].inference(cat, torch.LongTensor([cat.size(1)]).to(cond.device), bundle["ref_mel"], bundle["style"],
                                                  None, 25, inference_cfg_rate=0.7)[:, :, bundle["ref_mel"].size(-1):]
            mels.append(mel.float())
            lens.append(mel.shape[-1])
        out = torch.zeros(len(mels), mels[0].shape[1], max(lens), device=codes.device)
        for b, m in enumerate(mels):
            out[b, :, : lens[b]] = m[0]
        return out, torch.tensor(lens, dtype=torch.int32)
