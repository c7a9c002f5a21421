"""In-process serving shell: a speaker-bundle cache keyed by the prompt audio's bytes and a dynamic
batcher that turns concurrent single-utterance requests into `IndexTTS2.infer_batch` calls -- the pieces of the reference's
Triton front end that decide WHAT runs as one batch (`SpeakerCache`, backends/trt/serving/triton_server.py:44-94; the `@batch`
decorated `infer_non_streaming`, :170-230), without its network layer.  `infer_batch` batches utterances of ONE speaker bundle, so by
default requests are grouped by (speaker prompt, emotion prompt, emo_alpha, language, generation settings); with `mixed=True` requests
of different voices and different sampling settings share `IndexTTS2.infer_requests` batches (per-request settings in one batch,
triton_server.py:96-305) and only the call-wide settings group them.  `StreamBatcher` is the streaming counterpart: concurrent callers
share one `IndexTTS2.stream_session`, each reading its own stream's pieces as they are rendered."""
import collections
import hashlib
import queue
import threading
import time
from concurrent.futures import Future
from typing import Any, Callable, Dict, Hashable, List, Optional, Tuple


class SpeakerCache:
    """LRU of computed speaker bundles keyed by a hash of the prompt audio (bytes or a path): the prompt encoders run once per
    distinct prompt (triton_server.py:44-94)."""

    def __init__(self, compute: Callable[[Any], Any], max_size: int = 64):
        self.compute, self.max_size = compute, int(max_size)
        self._d: "collections.OrderedDict[str, Any]" = collections.OrderedDict()
        self._lock = threading.Lock()
        self.hits = self.misses = 0

    @staticmethod
    def key_of(audio) -> str:
        data = audio if isinstance(audio, (bytes, bytearray, memoryview)) else str(audio).encode()
        return hashlib.sha256(bytes(data)).hexdigest()

    def get_or_compute(self, audio):
        k = self.key_of(audio)
        with self._lock:
            if k in self._d:
                self._d.move_to_end(k)
                self.hits += 1
                return self._d[k]
        v = self.compute(audio)                      # outside the lock: prompt encoders take a while
        with self._lock:
            self.misses += 1
            self._d[k] = v
            self._d.move_to_end(k)
            while len(self._d) > self.max_size:
                self._d.popitem(last=False)
        return v

    def get_or_compute_many(self, audios, compute_many: Callable[[List[Any]], List[Any]]) -> List[Any]:
        """`get_or_compute` for a list: hits come from the cache, the DISTINCT misses go to ONE `compute_many(list)` call (first-appearance
        order, outside the lock), duplicates are computed once, results come back in input order.  `hits` / `misses` count what a loop of
        `get_or_compute` over the list would count; the LRU bound holds."""
        audios = list(audios)
        keys = [self.key_of(a) for a in audios]
        found: Dict[str, Any] = {}
        todo: "collections.OrderedDict[str, Any]" = collections.OrderedDict()
        with self._lock:
            for k, a in zip(keys, audios):
                if k in self._d:
                    self._d.move_to_end(k)
                    found[k] = self._d[k]
                elif k not in todo:
                    todo[k] = a
        if todo:
            vals = list(compute_many(list(todo.values())))
            if len(vals) != len(todo):
                raise RuntimeError(f"SpeakerCache: compute_many returned {len(vals)} results for {len(todo)} prompts")
            found.update(zip(todo.keys(), vals))
        with self._lock:
            self.misses += len(todo)
            self.hits += len(keys) - len(todo)
            for k in todo:
                self._d[k] = found[k]
                self._d.move_to_end(k)
            while len(self._d) > self.max_size:
                self._d.popitem(last=False)
        return [found[k] for k in keys]


# generation settings a request of a mixed batch may carry for itself (`IndexTTS2.infer_requests`); every other kwarg is call-wide
PER_REQUEST_SETTINGS = ("top_p", "top_k", "temperature", "repetition_penalty", "max_mel_tokens", "seed", "typical_sampling", "typical_mass")
# codes -> mel settings of a request (`infer_requests`): per request under any beam mode, so never part of a mixed batch's group key.  `cfm_noise`
# is call-wide: it stays among the kwargs that key the group and reaches `infer_requests` / `infer_batch` with them
PER_REQUEST_S2MEL = ("diffusion_steps", "inference_cfg_rate", "cfm_temperature")
# logits filters of a request (`infer_requests`: the engine's per-slot filter table): per request where the sampling settings are -- num_beams = 1
# or beam_settings="own" -- and only for a batcher opened with request_filters=True; otherwise they key the group like any other kwarg.
# (`gpt._LOGITS_FILTER_KWARGS`, restated so that this module imports without the engine; tests/test_row_filters_host.py holds the two equal.)
PER_REQUEST_FILTERS = ("no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens",
                       "epsilon_cutoff", "eta_cutoff", "exponential_decay_length_penalty", "min_p")


class _Request:
    __slots__ = ("group", "text", "future", "t", "req")

    def __init__(self, group, text, req=None):
        self.group, self.text, self.future, self.t, self.req = group, text, Future(), time.monotonic(), req


class DynamicBatcher:
    """submit(...) returns a Future of `(sample_rate, int16 array)`; a worker thread collects the requests of one group until
    `max_batch` of them wait or the oldest has waited `max_wait_ms`, and runs them as ONE `infer_batch` call.  Groups are served
    oldest-first; a failing batch fails exactly its own futures."""

    def __init__(self, tts, max_batch: int = 64, max_wait_ms: float = 10.0, inflight_slots: Optional[int] = None,
                 inflight_beam_slots: Optional[int] = None, mixed: bool = False, request_filters: bool = False):
        """request_filters (with mixed): the logits-filter kwargs (`PER_REQUEST_FILTERS`) leave the group key and travel with the request, under
        the condition the sampling settings do (num_beams = 1, or `beam_settings="own"`): requests that differ only in, say, `min_new_tokens`
        then share a batch.  Default False: they key the group, as every other kwarg.
        mixed: requests of different voices, languages, emotion prompts and -- with num_beams = 1 -- different sampling settings
        (`PER_REQUEST_SETTINGS`) run as ONE `tts.infer_requests` call; the group key shrinks to the call-wide settings (`num_beams`,
        `length_penalty`, `beam_settings`, any other kwarg, and the sampling settings when num_beams > 1 unless `beam_settings="own"` is
        submitted with the request: then `infer_requests` keeps them per request under beam search too).
        inflight_slots: decode at most that many rows at a time and admit the batch's waiting utterances into the slots of rows that have
        stopped (`UnifiedVoice.inference_speech_inflight`, num_beams = 1) -- `max_batch` can then exceed what one decode batch should hold.
        inflight_beam_slots: the same for requests that search with beams (`num_beams` > 1, the default 3): that many beam groups search at a
        time and finished groups are refilled (`UnifiedVoice.inference_speech_inflight_beams`)."""
        self.tts, self.max_batch, self.max_wait = tts, int(max_batch), float(max_wait_ms) / 1000.0
        self.inflight_slots = None if not inflight_slots else int(inflight_slots)
        self.inflight_beam_slots = None if not inflight_beam_slots else int(inflight_beam_slots)
        self.mixed = bool(mixed)
        self.request_filters = bool(request_filters)
        self._q: List[_Request] = []
        self._cv = threading.Condition()
        self._stop = False
        self.batches: List[int] = []                 # size of every batch that ran (observability / tests)
        self._worker = threading.Thread(target=self._run, name="indextts-batcher", daemon=True)
        self._worker.start()

    def submit(self, spk_audio_prompt, text: str, lang, emo_audio_prompt=None, emo_alpha: float = 1.0, **generation_kwargs) -> Future:
        """`audio_format=` (`output.AudioFormat`, a dict or "rate/encoding"): the Future's result is `(the format's rate, array of its dtype)`.
        The format is part of the group key, so a batch shares one; with `mixed` it travels with the request (`infer_requests` groups the
        requests of a batch by format for the conversion)."""
        fmt = None
        if generation_kwargs.get("audio_format") is not None:
            from .output import AudioFormat
            fmt = AudioFormat.parse(generation_kwargs["audio_format"])     # checked here: a bad value goes to its caller; hashable for the key
        generation_kwargs = {k: v for k, v in generation_kwargs.items() if k != "audio_format"}
        if fmt is not None and not self.mixed:
            generation_kwargs["audio_format"] = fmt
        if self.mixed:
            own = {k: v for k, v in generation_kwargs.items() if k in PER_REQUEST_SETTINGS}
            if fmt is not None:
                own["audio_format"] = fmt
            s2 = {k: v for k, v in generation_kwargs.items() if k in PER_REQUEST_S2MEL}
            wide = {k: v for k, v in generation_kwargs.items() if k not in PER_REQUEST_SETTINGS and k not in PER_REQUEST_S2MEL}
            # settings a batch must share stay in the group key: the per-request ones under beams, unless the call keeps them per request
            per_request = wide.get("num_beams", 3) == 1 or wide.get("beam_settings", "shared") == "own"
            filt = {}
            if self.request_filters and per_request:
                filt = {k: v for k, v in wide.items() if k in PER_REQUEST_FILTERS}
                wide = {k: v for k, v in wide.items() if k not in PER_REQUEST_FILTERS}
            key = ("mixed", tuple(sorted(wide.items())), () if per_request else tuple(sorted((k, v) for k, v in own.items() if k != "audio_format")))
            req = dict(spk_audio_prompt=spk_audio_prompt, text=text, lang=lang, emo_audio_prompt=emo_audio_prompt, emo_alpha=emo_alpha, **own, **s2,
                       **filt)
            r = _Request((key, wide), text, req)
            with self._cv:
                if self._stop:
                    raise RuntimeError("DynamicBatcher is closed")
                self._q.append(r)
                self._cv.notify()
            return r.future
        group: Tuple[Hashable, ...] = (SpeakerCache.key_of(spk_audio_prompt), None if emo_audio_prompt is None else SpeakerCache.key_of(emo_audio_prompt),
                                       float(emo_alpha), lang, tuple(sorted(generation_kwargs.items())))
        r = _Request((group, spk_audio_prompt, emo_audio_prompt), text)
        with self._cv:
            if self._stop:
                raise RuntimeError("DynamicBatcher is closed")
            self._q.append(r)
            self._cv.notify()
        return r.future

    def close(self):
        with self._cv:
            self._stop = True
            self._cv.notify()
        self._worker.join()

    def _take(self) -> Optional[List[_Request]]:
        with self._cv:
            while True:
                if self._q:
                    head = self._q[0]
                    same = [r for r in self._q if r.group[0] == head.group[0]]
                    wait = self.max_wait - (time.monotonic() - head.t)
                    if len(same) >= self.max_batch or wait <= 0 or self._stop:
                        take = same[: self.max_batch]
                        ids = {id(r) for r in take}
                        self._q = [r for r in self._q if id(r) not in ids]
                        return take
                    self._cv.wait(timeout=wait)
                elif self._stop:
                    return None
                else:
                    self._cv.wait()

    def _run(self):
        while True:
            reqs = self._take()
            if reqs is None:
                return
            self.batches.append(len(reqs))
            try:
                if self.mixed:
                    gen = dict(reqs[0].group[1])
                else:
                    (key, spk, emo) = reqs[0].group
                    _, _, emo_alpha, lang, gen = key
                    gen = dict(gen)
                if self.inflight_slots and gen.get("num_beams", 3) == 1:
                    gen.setdefault("inflight_slots", self.inflight_slots)
                if self.inflight_beam_slots and gen.get("num_beams", 3) > 1:
                    gen.setdefault("inflight_beam_slots", self.inflight_beam_slots)
                if self.mixed:
                    res = list(self.tts.infer_requests([r.req for r in reqs], **gen))
                else:
                    res = list(self.tts.infer_batch(spk, [r.text for r in reqs], lang, emo_audio_prompt=emo, emo_alpha=emo_alpha, **gen))
                if len(res) != len(reqs):
                    raise RuntimeError(f"{'infer_requests' if self.mixed else 'infer_batch'} returned {len(res)} results for {len(reqs)} requests")
                for r, out in zip(reqs, res):
                    if r.future.set_running_or_notify_cancel():      # a caller may have cancelled while the batch ran
                        r.future.set_result(out)
            except Exception as e:                    # noqa: BLE001 -- delivered to the callers of this batch
                for r in reqs:
                    if not r.future.done():
                        try:
                            r.future.set_exception(e)
                        except Exception:             # noqa: BLE001 -- cancelled in between: nobody is waiting
                            pass


class _PieceStream:
    """What `StreamBatcher.submit` returns: an iterator of `(22050, int16 array)` pieces that ends when the stream is done (or was cancelled,
    or the batcher was closed without draining); a request the session refused raises its error here."""
    _END = object()

    def __init__(self, batcher):
        self._batcher, self._q, self._over = batcher, queue.Queue(), False

    def __iter__(self):
        return self

    def __next__(self):
        if self._over:
            raise StopIteration
        item = self._q.get()
        if item is self._END:
            self._over = True
            raise StopIteration
        if isinstance(item, BaseException):
            self._over = True
            raise item
        return item

    def cancel(self):
        self._batcher.cancel(self)


class StreamBatcher:
    """Concurrent streaming requests over ONE `tts.stream_session(slots=..., **session_kwargs)`: `submit(**request)` is thread-safe and returns
    an iterator of the stream's `(22050, int16)` pieces (with an `audio_format` key in the request, or as a session default: the format's rate
    and dtype); one worker thread owns the session -- it submits what arrived, steps the session and
    hands every piece to its stream's iterator.  `cancel(stream)` (or `stream.cancel()`) stops a stream; `close()` stops accepting, lets the
    live and waiting streams finish (as `DynamicBatcher.close` serves what was queued; `drain=False` ends them at once), releases the engine
    and ends every iterator."""

    def __init__(self, tts, slots: int, **session_kwargs):
        self._session = tts.stream_session(slots=slots, **session_kwargs)
        self._cv = threading.Condition()
        self._inbox: List[Tuple[str, Any, Any]] = []       # ("submit", request, stream) / ("cancel", None, stream), in arrival order
        self._stop = self._drain = False
        self._by_id: Dict[int, _PieceStream] = {}
        self._worker = threading.Thread(target=self._run, name="indextts-stream-batcher", daemon=True)
        self._worker.start()

    @property
    def stats(self):
        return self._session.stats

    def submit(self, **request) -> _PieceStream:
        stream = _PieceStream(self)
        with self._cv:
            if self._stop:
                raise RuntimeError("StreamBatcher is closed")
            self._inbox.append(("submit", request, stream))
            self._cv.notify()
        return stream

    def cancel(self, stream: _PieceStream):
        with self._cv:
            self._inbox.append(("cancel", None, stream))
            self._cv.notify()

    def close(self, drain: bool = True):
        with self._cv:
            self._stop, self._drain = True, bool(drain)
            self._cv.notify()
        self._worker.join()

    def _run(self):
        sess = self._session
        try:
            while True:
                with self._cv:
                    while not self._inbox and not self._stop and not sess.active:
                        self._cv.wait()
                    inbox, self._inbox = self._inbox, []
                    if self._stop and not inbox and not (self._drain and sess.active):
                        return
                for what, request, stream in inbox:
                    if what == "submit":
                        try:
                            self._by_id[sess.submit(request)] = stream
                        except Exception as e:            # noqa: BLE001 -- delivered to the caller of this request
                            stream._q.put(e)
                    else:
                        for sid in [k for k, v in self._by_id.items() if v is stream]:
                            sess.cancel(sid)
                for sid, sr, piece, done, _ in sess.step():
                    stream = self._by_id.get(sid)
                    if stream is None:
                        continue
                    if piece is not None:
                        stream._q.put((sr, piece))
                    if done:
                        stream._q.put(_PieceStream._END)
                        del self._by_id[sid]
        except Exception as e:                            # noqa: BLE001 -- the session failed: every open stream gets the error
            for stream in self._by_id.values():
                stream._q.put(e)
            self._by_id.clear()
        finally:
            with self._cv:
                self._stop = True
                late, self._inbox = self._inbox, []
            for what, _, stream in late:
                if what == "submit":
                    stream._q.put(_PieceStream._END)
            for stream in self._by_id.values():
                stream._q.put(_PieceStream._END)
            self._by_id.clear()
            sess.close()


def synthesize_tasks(tts, tasks: List[Dict[str, Any]], lang=None, max_batch: int = 64, mixed: bool = False, request_filters: bool = False,
                     **generation_kwargs) -> List[str]:
    """Batch-file synthesis (`_run_batch`, indextts/cli_v2.py:605-678, which calls `tts.infer` once per task): tasks that share
    the voice prompt and emotion settings run as real `infer_batch` batches of up to `max_batch` utterances; every task's audio
    is written to its own `output_path` (16-bit PCM WAV, `save_pcm_wav` semantics; with `audio_format=` -- call-wide, or a task key under
    `mixed` -- the delivery format's samples under the matching WAVE format tag, `output.save_audio_wav`).  A task is a dict with `voice_path`, `text`,
    `output_path` and optional `emotion_kwargs` (`emo_audio_prompt`, `emo_alpha`) / `line_number`, as `_load_batch_tasks` builds
    them.  mixed=True: tasks of DIFFERENT voices share `infer_requests` batches of up to `max_batch` tasks, in task order.
    request_filters=True (with mixed, where `infer_requests` keeps settings per request: num_beams = 1 or beam_settings="own"): a task's own
    logits-filter keys (`PER_REQUEST_FILTERS`, e.g. `min_new_tokens`) travel with its request instead of being ignored.
    Returns the written paths in task order; a failing batch raises with the line numbers it covered."""
    import os
    import torch
    from .infer_v2_5 import save_pcm_wav
    from .output import AudioFormat, save_audio_wav
    call_fmt = AudioFormat.parse(generation_kwargs.get("audio_format"))
    formats = [AudioFormat.parse(t.get("audio_format")) or call_fmt if mixed else call_fmt for t in tasks]
    groups: "collections.OrderedDict[Tuple, List[int]]" = collections.OrderedDict()
    written: List[Optional[str]] = [None] * len(tasks)

    def write(i, out):
        if out is None:
            return
        path = str(tasks[i]["output_path"])
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        sr, wav = out
        if formats[i] is None:
            save_pcm_wav(path, torch.from_numpy(wav.T.copy()).float(), sr)
        else:                                     # a delivery format: the encoded samples as they are, under the matching WAVE format tag
            save_audio_wav(path, wav, formats[i])
        written[i] = path
    if mixed:
        reqs = []
        per_request = generation_kwargs.get("num_beams", 3) == 1 or generation_kwargs.get("beam_settings", "shared") == "own"
        for i, t in enumerate(tasks):
            ek = dict(t.get("emotion_kwargs") or {})
            unsupported = set(ek) - {"emo_audio_prompt", "emo_alpha", "emo_vector"}
            if unsupported:
                raise ValueError(f"batch line {t.get('line_number', i + 1)}: {sorted(unsupported)} need the per-utterance infer() path")
            filt = {k: t[k] for k in PER_REQUEST_FILTERS if k in t} if request_filters and per_request else {}
            own_fmt = {"audio_format": t["audio_format"]} if t.get("audio_format") is not None else {}
            reqs.append(dict(spk_audio_prompt=str(t["voice_path"]), text=t["text"], lang=t.get("lang", lang), **ek, **filt, **own_fmt))
        for j in range(0, len(reqs), max_batch):
            part = list(range(j, min(j + max_batch, len(reqs))))
            try:
                res = tts.infer_requests([reqs[i] for i in part], **generation_kwargs)
            except Exception as e:                # noqa: BLE001
                lines = [tasks[i].get("line_number", i + 1) for i in part]
                raise RuntimeError(f"batch file lines {lines} inference failed: {e}") from e
            for i, out in zip(part, res):
                write(i, out)
        return written
    for i, t in enumerate(tasks):
        ek = dict(t.get("emotion_kwargs") or {})
        unsupported = set(ek) - {"emo_audio_prompt", "emo_alpha"}
        if unsupported:
            raise ValueError(f"batch line {t.get('line_number', i + 1)}: {sorted(unsupported)} need the per-utterance infer() path")
        key = (str(t["voice_path"]), None if ek.get("emo_audio_prompt") is None else str(ek["emo_audio_prompt"]), float(ek.get("emo_alpha", 1.0)))
        groups.setdefault(key, []).append(i)
    for (voice, emo, alpha), idx in groups.items():
        for j in range(0, len(idx), max_batch):
            part = idx[j: j + max_batch]
            try:
                res = tts.infer_batch(voice, [tasks[i]["text"] for i in part], lang, emo_audio_prompt=emo, emo_alpha=alpha, **generation_kwargs)
            except Exception as e:                # noqa: BLE001
                lines = [tasks[i].get("line_number", i + 1) for i in part]
                raise RuntimeError(f"batch file lines {lines} inference failed: {e}") from e
            for i, out in zip(part, res):
                write(i, out)
    return written
