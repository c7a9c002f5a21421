"""Streaming synthesis: chunked GPT emission -> per-chunk codes-to-audio -> Hann cross-fade.

Mirrors `StreamingDecoder` of the reference's TensorRT pipeline (`backends/trt/pipeline/streaming.py:57-210`): the GPT engine
yields chunks of `chunk_size` codes that overlap by `overlap_size` codes (`UnifiedVoice.generate_chunks`, the decode loop stays
suspended on the device between chunks); every chunk goes through codes -> mel -> waveform on its own, the overlapping samples
of consecutive chunks are cross-faded with the two halves of a Hann window, and every row's last piece gets a short linear
fade-out.  Yields `(sample_rate, audio_list, done_list)` per chunk with int16 arrays (None for rows that finished earlier).

The flow-matching stage attends over a whole chunk, so a chunked utterance is NOT sample-identical to the one-shot synthesis
(the reference's streaming mode has the same property); where exactness matters the vocoder alone can be streamed exactly
(`BigVGAN.stream` / `open_stream`, overlap-save with the receptive-field halo).

`StreamSession` is the open-ended form: streams are submitted one at a time, each with its own voice and settings, and join the decode batch
as soon as a slot is free ("Streaming sessions").  `RowStream` holds what one row of either form carries from chunk to chunk.
"""
import collections
import time
from typing import Callable, Dict, List, Optional

import numpy as np

MEL_CODE_TO_FRAME_RATIO = 1.72        # mel frames per code (infer_v2.py:662)
HOP_SIZE = 256
SAMPLE_RATE = 22050
PCM16_MAX = 32767
TAIL_FADE_SAMPLES = 512


def overlap_samples(n_codes: int, frames_per_code: float = MEL_CODE_TO_FRAME_RATIO) -> int:
    """samples covered by `n_codes` codes (streaming.py:13-14; the reference's ratio is IndexTTS-2's 1.72 frames per code -- the v2.5
    pipeline renders int(2 * n * 1.72 * duration_factor) frames for n codes, infer_v2_5.py:833, and passes that ratio)"""
    return int(n_codes * frames_per_code) * HOP_SIZE


def crossfade(tail: np.ndarray, head: np.ndarray) -> np.ndarray:
    """`tail` fading out into `head` over their common length with a Hann window's falling / rising halves (streaming.py:17-27)."""
    n = min(len(tail), len(head))
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    w = np.hanning(2 * n)
    return tail[:n] * w[n:] + head[:n] * w[:n]


def to_int16(audio: np.ndarray) -> np.ndarray:
    return np.clip(audio * PCM16_MAX, -PCM16_MAX, PCM16_MAX).astype(np.int16)


def fade_out_tail(audio: np.ndarray, fade_samples: int = TAIL_FADE_SAMPLES) -> np.ndarray:
    if len(audio) <= fade_samples:
        return audio
    out = audio.copy()
    out[-fade_samples:] *= np.linspace(1.0, 0.0, fade_samples)
    return out


class RowStream:
    """One row's chunk and cross-fade state.  Chunk k covers the row's codes [k * stride, k * stride + chunk_size); `due` names the chunks that
    can be rendered once `n_codes` codes before a stop token are known, `push` turns a rendered chunk into the piece to emit (the overlap with
    the previous chunk cross-faded, the samples the next chunk overlaps held back), `flush` emits what is still held back when the row ended
    without a closing chunk.  A row that ran into its token cap and a row that drew its own stop token after the same number of codes get the
    same chunks: a non-final chunk is due once all its codes exist, and the closing chunk is what lies past the last stride boundary."""

    def __init__(self, chunk_size: int, overlap_size: int, frames_per_code: float = MEL_CODE_TO_FRAME_RATIO):
        self.chunk_size, self.stride = int(chunk_size), int(chunk_size) - int(overlap_size)
        self.ovlp = overlap_samples(int(overlap_size), frames_per_code)
        self.next_chunk = 0                          # index of the next chunk to come
        self.tail: Optional[np.ndarray] = None       # samples still waiting for the next chunk's head
        self.finished = False

    def due(self, n_codes: int, ended: bool) -> List[tuple]:
        """[(chunk index, first code, number of codes, last)] of the chunks that became renderable: `n_codes` codes of the row are known and none
        of them is the stop token; `ended`: the row has no more to come (its stop token, or its cap)."""
        out = []
        while n_codes >= self.next_chunk * self.stride + self.chunk_size:
            out.append((self.next_chunk, self.next_chunk * self.stride, self.chunk_size, False))
            self.next_chunk += 1
        pos = self.next_chunk * self.stride
        if ended and pos < n_codes:                  # the closing chunk: what is left past the last boundary (at least the overlap)
            out.append((self.next_chunk, pos, n_codes - pos, True))
            self.next_chunk += 1
        return out

    def push(self, audio, last: bool) -> np.ndarray:
        """the int16 piece of the row's next rendered chunk (float32 samples in [-1, 1] covering that chunk's codes)"""
        audio, ovlp = np.asarray(audio, dtype=np.float32), self.ovlp
        if self.tail is None:                        # the row's first chunk
            piece, keep = (audio, None) if last else (audio[: len(audio) - ovlp], audio[len(audio) - ovlp:])
        else:
            rest = audio[ovlp:]
            blended = crossfade(self.tail, audio[:ovlp])
            if last:
                piece, keep = np.concatenate([blended, rest]), None
            else:
                piece, keep = np.concatenate([blended, rest[: len(rest) - ovlp]]), rest[len(rest) - ovlp:]
        if last:
            self.finished, self.tail = True, None
            return to_int16(fade_out_tail(piece))
        self.tail = keep
        return to_int16(piece)

    def flush(self) -> Optional[np.ndarray]:
        """the held-back samples as the row's last piece when it ended without a closing chunk, else None"""
        if self.tail is None or self.finished:
            return None
        self.finished = True
        return to_int16(fade_out_tail(self.tail))


class StreamingDecoder:
    """gpt_engine: an object with `generate_chunks(...)` yielding `(codes, is_last, batch_done, code_lens)` (UnifiedVoice);
    codes_to_audio_fn(codes, code_lens) -> list of float32 arrays in [-1, 1], one per row, covering that chunk's codes.  While the function
    runs, `chunk_index` is the index of the chunk it is rendering (what a per-chunk noise key reads)."""

    def __init__(self, gpt_engine, codes_to_audio_fn: Callable, chunk_size: int = 100, overlap_size: int = 20, verbose: bool = False,
                 frames_per_code: float = MEL_CODE_TO_FRAME_RATIO, audio_format=None):
        # audio_format (`output.AudioFormat`): codes_to_audio_fn returns DEVICE rows, and the cross-fade, the resampling and the encoding of
        # all rows run there (`output.deliver`); the items carry the format's rate and dtype.  None: the host path below, as always.
        self.audio_format = audio_format
        if overlap_size >= chunk_size:
            raise ValueError(f"overlap_size ({overlap_size}) must be less than chunk_size ({chunk_size})")
        if not frames_per_code > 0:
            raise ValueError(f"frames_per_code must be positive, got {frames_per_code}")
        self.frames_per_code = float(frames_per_code)     # mel frames codes_to_audio_fn renders per code: sizes the cross-fade
        self.gpt_engine, self.codes_to_audio_fn = gpt_engine, codes_to_audio_fn
        self.chunk_size, self.overlap_size = int(chunk_size), int(overlap_size)
        self.stride = self.chunk_size - self.overlap_size
        self.verbose = verbose
        self.first_chunk_latency: Optional[float] = None
        self.chunk_index = 0

    def generate(self, inputs_embeds, attention_mask, max_new_tokens: int = 1500, **generation_kwargs):
        B = inputs_embeds.shape[0]
        rows = [RowStream(self.chunk_size, self.overlap_size, self.frames_per_code) for _ in range(B)]
        outs, rate = None, SAMPLE_RATE
        if self.audio_format is not None:
            from . import output
            outs, rate = [output.OutputStream(self.audio_format, r.ovlp) for r in rows], self.audio_format.sample_rate
        t0 = time.perf_counter()
        self.first_chunk_latency = None
        for idx, (codes, is_last, batch_done, code_lens) in enumerate(self.gpt_engine.generate_chunks(
                inputs_embeds, attention_mask, max_new_tokens, self.chunk_size, self.overlap_size, **generation_kwargs)):
            self.chunk_index = idx
            audios = self.codes_to_audio_fn(codes, code_lens)
            if self.first_chunk_latency is None:
                self.first_chunk_latency = time.perf_counter() - t0
            if self.verbose:
                print(f">> [streaming] chunk {idx}: {codes.shape[1]} codes -> {len(audios[0])} samples")
            out: List[Optional[np.ndarray]] = [None] * B
            done = [False] * B
            live = [b for b, row in enumerate(rows) if not row.finished]
            for b in live:
                done[b] = bool(batch_done[b]) or is_last
            if outs is None:
                for b in live:
                    out[b] = rows[b].push(audios[b], done[b])
            else:                                        # all rows in one launch each of piece, resample, encode; one copy to the host
                for b, piece in zip(live, output.deliver([outs[b] for b in live], [audios[b] for b in live], [done[b] for b in live])):
                    out[b], rows[b].finished = piece, done[b]
            yield rate, out, done
        if outs is not None:
            if any(o.tail is not None and not o.finished for o in outs):
                out = output.deliver(outs, [None] * B, [True] * B)
                yield rate, out, [o is not None for o in out]
        elif any(r.tail is not None and not r.finished for r in rows):            # the engine stopped without a closing chunk
            out = [r.flush() for r in rows]
            yield SAMPLE_RATE, out, [o is not None for o in out]


_STOPPING = object()                                 # a slot whose cancelled row the engine has not stopped yet


class StreamSession:
    """An open-ended streaming batch: `submit(request)` at any time, `step()` for the audio that became due (`IndexTTS2.stream_session`).
    The scheduling lives here, on the host; everything that touches the engine is the `backend`:

      prepare(request) -> item                 validate and normalise a request (ValueError), encode its prompts
      frames_per_code(item) -> float           mel frames the item's codes render to, per code
      open(items)                              open the decode session; one item per slot, None for an empty slot (a row that ends at step 0)
      admit(slots, items)                      put items into slots whose rows have ended
      run(n, return_when_finished)             advance every live row by at most n steps
      steps                                    the session's step count
      progress() -> [(n_codes, ended)]         per slot: codes before a stop token so far, and whether the row has ended
      stop(slot)                               end the slot's row at the engine's next step
      collect(jobs) -> windows                 copy the code windows of jobs [(item, slot, chunk index, first code, number of codes)]
      render(jobs, windows) -> [float32 array] the windows' audio, one array per job: ONE codes -> mel call and ONE ragged vocoder call
                                               (a DEVICE row for a job whose item carries an `audio_format`: see below)
      close()

    An item with an `audio_format` attribute (`output.AudioFormat`) is delivered in that format: its rows stay on the device, and the cross-fade,
    the streaming resampler and the encoding of all such jobs of a render run there (`output.deliver`); its events carry the format's rate and
    dtype.  Items without one go through `RowStream.push` on the host, as always; both kinds share a session.

    A stream's events do not depend on its slot, the step it joined at, its batch mates or `poll_steps`: chunk k is always the row's own codes
    [k * stride, k * stride + chunk_size), rendered at the first poll at or after the step that completed it."""

    def __init__(self, backend, slots: int, chunk_size: int = 100, overlap_size: int = 20, poll_steps: int = 8):
        if int(slots) < 1:
            raise ValueError(f"slots must be >= 1, got {slots}")
        if overlap_size >= chunk_size or overlap_size < 0:
            raise ValueError(f"overlap_size ({overlap_size}) must be >= 0 and less than chunk_size ({chunk_size})")
        if int(poll_steps) < 1:
            raise ValueError(f"poll_steps must be >= 1, got {poll_steps}")
        self.backend, self.slots = backend, int(slots)
        self.chunk_size, self.overlap_size, self.poll_steps = int(chunk_size), int(overlap_size), int(poll_steps)
        self._waiting: "collections.deque" = collections.deque()       # (stream id, item), FIFO
        self._busy: list = [None] * self.slots       # per slot: the stream id it serves, _STOPPING, or None (free: its row has ended)
        self._streams: Dict[int, dict] = {}          # live streams: item, row state, slot
        self._pending: List[tuple] = []              # events made outside step() (cancel), delivered by the next step()
        self._next_id = 0
        self._opened = self._closed = False
        # per stream: `admitted_step` / `slot` it was admitted at, `first_audio_s` from submit to its first piece; per render call its rows
        self.stats = dict(streams={}, render_rows=[])

    # ---- the public surface ----------------------------------------------------------------------------------------------------------
    def submit(self, request: dict) -> int:
        if self._closed:
            raise RuntimeError("StreamSession.submit: the session is closed")
        item = self.backend.prepare(request)
        sid, self._next_id = self._next_id, self._next_id + 1
        self._waiting.append((sid, item))
        self.stats["streams"][sid] = dict(submitted=time.perf_counter(), admitted_step=None, slot=None, first_audio_s=None)
        return sid

    @property
    def active(self) -> bool:
        """something is live, waiting, or still to be reported"""
        return bool(self._waiting or self._pending or any(b is not None for b in self._busy))

    def cancel(self, sid: int) -> bool:
        """stop a stream: its slot is free once the engine has stopped the row (its next step), a waiting request just leaves the queue; the
        stream gets one final `done` event without audio.  False when the stream is not live or waiting (any more)."""
        for i, (w, item) in enumerate(self._waiting):
            if w == sid:
                del self._waiting[i]
                self._pending.append((sid, self._rate(item), None, True, 0))
                return True
        st = self._streams.pop(sid, None)
        if st is None:
            return False
        self.backend.stop(st["slot"])
        self._busy[st["slot"]] = _STOPPING
        self._pending.append((sid, self._rate(st["item"]), None, True, st["row"].next_chunk))
        return True

    @staticmethod
    def _rate(item) -> int:
        """the rate a stream's events carry: its `audio_format`'s (an item prepared with one is delivered by `output.deliver`), else 22050"""
        fmt = getattr(item, "audio_format", None)
        return SAMPLE_RATE if fmt is None else fmt.sample_rate

    def _deliver(self, sids, audios, lasts):
        """the pieces of streams with an `audio_format`, made on the device: all of them in one `output.deliver` call -- in as many as its
        busiest stream has jobs when a long poll completed several chunks of one stream"""
        from . import output
        pieces, todo = [None] * len(sids), list(range(len(sids)))
        while todo:
            batch, later, seen = [], [], set()
            for n in todo:
                (later if sids[n] in seen else batch).append(n)
                seen.add(sids[n])
            got = output.deliver([self._streams[sids[n]]["out"] for n in batch], [audios[n] for n in batch], [lasts[n] for n in batch])
            for n, piece in zip(batch, got):
                pieces[n] = piece
            todo = later
        return pieces

    def step(self) -> List[tuple]:
        """advance the decode session by at most `poll_steps` steps, refill freed slots, render what became due.  -> events
        (stream id, 22050, int16 array or None, done, chunk index), per stream in chunk order (a stream with an `audio_format`: its rate and
        dtype)."""
        if self._closed:
            raise RuntimeError("StreamSession.step: the session is closed")
        events, self._pending = self._pending, []
        if not self._opened:
            if not self._waiting:
                return events
            take = [self._waiting.popleft() for _ in range(min(self.slots, len(self._waiting)))]
            self.backend.open([it for _, it in take] + [None] * (self.slots - len(take)))
            self._opened = True
            for slot, (sid, item) in enumerate(take):
                self._place(slot, sid, item)
            for slot in range(len(take), self.slots):
                self._busy[slot] = _STOPPING         # an empty slot's row ends at step 0: free from the first poll on
        else:
            self._refill()
        if any(b is not None for b in self._busy):
            self.backend.run(self.poll_steps, 1 if self._waiting else 0)
        jobs, ended = [], []
        for slot, (n_codes, row_ended) in enumerate(self.backend.progress()):
            sid = self._busy[slot]
            if sid is _STOPPING:
                if row_ended:
                    self._busy[slot] = None
                continue
            if sid is None:
                continue
            st = self._streams[sid]
            jobs += [(sid, (st["item"], slot, k, pos, n), last) for k, pos, n, last in st["row"].due(n_codes, row_ended)]
            if row_ended:
                ended.append(sid)
                self._busy[slot] = None
        windows = self.backend.collect([j for _, j, _ in jobs]) if jobs else None      # before a refill overwrites an ended row's codes
        self._refill()
        if jobs:
            self.stats["render_rows"].append(len(jobs))
            audios = self.backend.render([j for _, j, _ in jobs], windows)
            now = time.perf_counter()
            dev = [n for n, (sid, _, _) in enumerate(jobs) if self._streams[sid]["out"] is not None]
            made = dict(zip(dev, self._deliver([jobs[n][0] for n in dev], [audios[n] for n in dev], [jobs[n][2] for n in dev]))) if dev else {}
            for n, ((sid, job, last), audio) in enumerate(zip(jobs, audios)):
                st = self._streams[sid]
                if n in made:
                    piece, st["row"].finished = made[n], st["row"].finished or last
                else:
                    piece = st["row"].push(audio, last)
                events.append((sid, self._rate(st["item"]), piece, last, job[2]))
                rec = self.stats["streams"][sid]
                if rec["first_audio_s"] is None:
                    rec["first_audio_s"] = now - rec["submitted"]
        flush = [sid for sid in ended if self._streams[sid]["out"] is not None and not self._streams[sid]["row"].finished]
        flushed = dict(zip(flush, self._deliver(flush, [None] * len(flush), [True] * len(flush)))) if flush else {}
        for sid in ended:
            st = self._streams.pop(sid)
            row = st["row"]
            if not row.finished:                     # no closing chunk: the held-back samples (or nothing at all) end the stream
                events.append((sid, self._rate(st["item"]), flushed[sid] if sid in flushed else row.flush(), True, row.next_chunk))
        return events

    def events(self):
        """iterate `step()` until nothing is live or waiting; `submit` and `cancel` may be called between two events"""
        while self.active:
            yield from self.step()

    def close(self):
        if not self._closed:
            self._closed = True
            if self._opened:
                self.backend.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- slots ------------------------------------------------------------------------------------------------------------------------
    def _place(self, slot: int, sid: int, item):
        self._busy[slot] = sid
        row, out = RowStream(self.chunk_size, self.overlap_size, self.backend.frames_per_code(item)), None
        if getattr(item, "audio_format", None) is not None:          # its pieces are made on the device (`_deliver`)
            from . import output
            out = output.OutputStream(item.audio_format, row.ovlp)
        self._streams[sid] = dict(item=item, slot=slot, row=row, out=out)
        self.stats["streams"][sid].update(admitted_step=int(self.backend.steps), slot=slot)

    def _refill(self):
        free = [s for s in range(self.slots) if self._busy[s] is None]
        if not free or not self._waiting:
            return
        take = [self._waiting.popleft() for _ in range(min(len(free), len(self._waiting)))]
        free = free[:len(take)]
        self.backend.admit(free, [it for _, it in take])
        for slot, (sid, item) in zip(free, take):
            self._place(slot, sid, item)
