"""Delivery formats: the vocoder's 22.05 kHz f32 rows resampled and encoded on the device.

Every pipeline entry used to end on the host: one `.cpu()` per segment row, `torch.cat` of the interval silences, `.type(torch.int16)`, and for
streams a numpy cross-fade per chunk -- always `(22050, int16)`.  With `audio_format=` a request names what it wants delivered instead:

    AudioFormat(sample_rate=8000, encoding="mulaw")      "8000/mulaw"      dict(sample_rate=48000, encoding="pcm_f32le", peak_dbfs=-1.0)

and the tail runs as four kernels of csrc/pcm_kernels.hip over packed ragged sequences (include/indextts_hip.h, "delivery formats"):

  itts_pcm_stream_piece_seq_forward   RowStream.push / flush for all jobs of a render (also the ragged copy that assembles a request)
  itts_pcm_resample_seq_forward       rational polyphase resampler, one-shot and streaming
  itts_pcm_peak_seq_forward           per-sequence max |x| for `peak_dbfs`
  itts_pcm_encode_seq_forward         gain, then pcm_s16le / mulaw / alaw / pcm_f32le

followed by ONE device-to-host copy per call and format.  A format with `loudness_lufs` (csrc/loudness_kernels.hip) puts
  itts_pcm_loudness_seq_forward       integrated loudness after ITU-R BS.1770-4 per sequence, f64, and its peak
  itts_pcm_loudness_gain_forward      (loudness, peak, target, ceiling) -> the encoder's per-sequence gain
between the resampler and the encoder.  A format with `limit_dbfs` / `true_peak` (csrc/limiter_kernels.hip) adds
  itts_pcm_truepeak_seq_forward       per-sequence true peak: max |u| of the 4x oversampled sequence, which is never written
  itts_pcm_limiter_seq_forward        look-ahead limiter, one-shot and streaming: the smoothed minimum of the gain each sample needs
the limiter between gain formation and the encoder, which then runs with gain 1.

The resampler.  g = gcd(orig, new), M = orig / g, L = new / g, fc = min(orig, new) / 2, fs_hi = orig * L, H = ceil(Z * fs_hi / (2 fc)), Z = 24:
    h[n] = L * (2 fc / fs_hi) * sinc(2 fc n / fs_hi) * kaiser(2H + 1, beta = 10)[n + H],   -H <= n <= H     (f64, rounded once to f32)
    y[m] = sum over i of h[m*M - i*L] * x[i],   i ascending over |m*M - i*L| <= H, 0 <= i < N          (one f32 fmaf chain from 0.f)
    N_out = ceil(N * L / M)
A stream's non-final call produces the outputs whose whole support has arrived, m*M + H < n_in*L; the final call the rest, zero-extended.  The
counts and the carried history are integer functions of (n_in, n_out) below; a stream's pieces concatenate to the bits of the one-shot call.
"""
import math
import re
import struct
from typing import List, Optional, Sequence

import numpy as np

SOURCE_RATE = 22050                   # what the vocoder renders
ZERO_CROSSINGS = 24                   # Z: one-sided prototype length in zero crossings of the sinc
KAISER_BETA = 10.0
TABLE_MAX_BYTES = 1 << 20             # ITTS_PCM_TABLE_MAX_BYTES
TAIL_FADE_SAMPLES = 512               # ITTS_PCM_TAIL_FADE
RESAMPLE_TILE = 1024                  # ITTS_PCM_RESAMPLE_TILE: consecutive outputs of one sequence a block serves
LOUDNESS_MIN_LUFS = -70.0             # the absolute gate of BS.1770: no target below it can be met
LOUDNESS_MIN_RATE, LOUDNESS_MAX_RATE = 4000, 384000                                       # ITTS_PCM_LOUDNESS_MIN_RATE / _MAX_RATE
LOUDNESS_WS_DOUBLES = 9               # ITTS_PCM_LOUDNESS_WS_DOUBLES
_LUFS_PART = re.compile(r"^([-+]?\d+(?:\.\d+)?)\s*lufs$", re.IGNORECASE)
_LIMIT_PART = re.compile(r"^([-+]?\d+(?:\.\d+)?)\s*limit$", re.IGNORECASE)
LIMITER_TILE = 1024                   # ITTS_PCM_LIMITER_TILE
LIMITER_MAX_LOOKAHEAD = 1024          # ITTS_PCM_LIMITER_MAX_LOOKAHEAD
ENCODINGS = {"pcm_s16le": 0, "mulaw": 1, "alaw": 2, "pcm_f32le": 3}                     # ITTS_PCM_*
DTYPES = {"pcm_s16le": np.int16, "mulaw": np.uint8, "alaw": np.uint8, "pcm_f32le": np.float32}
WAV_TAGS = {"pcm_s16le": 1, "pcm_f32le": 3, "alaw": 6, "mulaw": 7}                      # WAVE_FORMAT_PCM / IEEE_FLOAT / ALAW / MULAW


# ---- integer arithmetic of the resampler ------------------------------------------------------------------------------------------------
def resample_params(orig: int, new: int):
    """-> (L, M, H, K): up factor, down factor, one-sided prototype length at the rate orig * L, taps per phase K = ceil((2H + 1) / L)"""
    orig, new = int(orig), int(new)
    if orig < 1 or new < 1:
        raise ValueError(f"sample rates must be positive, got {orig} -> {new}")
    g = math.gcd(orig, new)
    M, L = orig // g, new // g
    H = -(-ZERO_CROSSINGS * orig * L // min(orig, new))          # ceil(Z * fs_hi / (2 fc)), 2 fc = min(orig, new)
    return L, M, H, (2 * H + L) // L


def rate_supported(orig: int, new: int) -> bool:
    """a pair is supported when its coefficient table (K * L f32) is at most 1 MiB"""
    L, _, _, K = resample_params(orig, new)
    return K * L * 4 <= TABLE_MAX_BYTES


def resampled_length(n_in: int, L: int, M: int) -> int:
    return -(-int(n_in) * L // M)


def outputs_ready(n_in: int, final: bool, L: int, M: int, H: int) -> int:
    """outputs 0 .. ready - 1 can be produced once n_in samples of the stream are known: every m with m*M + H < n_in*L, or all
    ceil(n_in*L / M) on the final call"""
    if final:
        return resampled_length(n_in, L, M)
    top = int(n_in) * L - H - 1
    return top // M + 1 if top >= 0 else 0


def first_needed(m: int, n_in: int, L: int, M: int, H: int) -> int:
    """the earliest input output m reads: ceil((m*M - H) / L), clipped to 0 .. n_in -- what a stream must carry from there on"""
    return min(max(0, -((H - int(m) * M) // L)), int(n_in))


# ---- integer arithmetic of the limiter -----------------------------------------------------------------------------------------------------
def limiter_lookahead(rate: int) -> int:
    """La = (rate * 5 + 500) // 1000 samples, about 5 ms (itts_pcm_limiter_lookahead); the limiter needs 1 <= La <= 1024"""
    return (int(rate) * 5 + 500) // 1000 if int(rate) >= 1 else 0


def limiter_reach(rate: int, true_peak: bool) -> int:
    """R: how far on either side of an output the limiter reads its stream -- La, and the prototype's Z more under `true_peak`"""
    return limiter_lookahead(rate) + (ZERO_CROSSINGS if true_peak else 0)


def limiter_ready(n_in: int, final: bool, R: int) -> int:
    """outputs 0 .. ready - 1 can be produced once n_in samples of the stream are known: every n with n + R < n_in, or all n_in on the final call"""
    return int(n_in) if final else max(0, int(n_in) - int(R))


def limiter_first_needed(n_out: int, R: int) -> int:
    """the earliest sample output n_out reads: max(0, n_out - R) -- what a stream must carry from there on"""
    return max(0, int(n_out) - int(R))


def limiter_taps(rate: int) -> np.ndarray:
    """w[k] proportional to sin^2(pi (k + 1) / (La + 2)), k = 0 .. La, normalised to sum 1 in f64 and rounded once to f32"""
    La = limiter_lookahead(rate)
    if not 1 <= La <= LIMITER_MAX_LOOKAHEAD:
        raise ValueError(f"limit_dbfs: the look-ahead at sample_rate {rate} is {La} samples; it must lie in [1, {LIMITER_MAX_LOOKAHEAD}]")
    w = np.sin(np.pi * (np.arange(La + 1, dtype=np.float64) + 1.0) / (La + 2.0)) ** 2
    return (w / w.sum()).astype(np.float32)


# ---- the prototype and its device table ---------------------------------------------------------------------------------------------------
def prototype(orig: int, new: int) -> np.ndarray:
    """h[-H .. H] in f64 (the docstring's definition)"""
    L, _, H, _ = resample_params(orig, new)
    two_fc, fs_hi = float(min(orig, new)), float(orig) * L
    n = np.arange(-H, H + 1, dtype=np.float64)
    return L * (two_fc / fs_hi) * np.sinc(two_fc * n / fs_hi) * np.kaiser(2 * H + 1, KAISER_BETA)


def phase_table(orig: int, new: int) -> np.ndarray:
    """the f32 prototype laid out by output residue, [K][L]: table[k][m mod L] = h[m*M - (ceil((m*M - H) / L) + k) * L], 0 outside [-H, H].  The lanes
    of a wave serve consecutive outputs, so they read consecutive coefficients."""
    L, M, H, K = resample_params(orig, new)
    h = prototype(orig, new).astype(np.float32)
    r = np.arange(L, dtype=np.int64)
    i_lo = -((H - r * M) // L)
    n = (r * M)[None, :] - (i_lo[None, :] + np.arange(K, dtype=np.int64)[:, None]) * L
    ok = np.abs(n) <= H
    return np.where(ok, h[np.clip(n + H, 0, 2 * H)], np.float32(0)).astype(np.float32)


_tables = {}


def resample_table(orig: int, new: int, device):
    """the device copy of `phase_table`, cached per (orig, new, device)"""
    import torch
    device = torch.device(device)
    key = (int(orig), int(new), str(device))
    if key not in _tables:
        if not rate_supported(orig, new):
            raise ValueError(f"resampling {orig} -> {new} Hz needs a coefficient table above {TABLE_MAX_BYTES} bytes")
        _tables[key] = torch.from_numpy(phase_table(orig, new)).to(device).contiguous()
    return _tables[key]


def limiter_window(rate: int, device):
    """the device copy of `limiter_taps`, cached per (rate, device) beside the resampling tables"""
    import torch
    device = torch.device(device)
    key = ("limiter", int(rate), str(device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(limiter_taps(rate)).to(device).contiguous()
    return _tables[key]


_windows = {}


def _window(n: int, device):
    """np.hanning(2n) as f32 on the device: rising half, then falling half"""
    import torch
    key = (int(n), str(device))
    if key not in _windows:
        if len(_windows) > 64:
            _windows.clear()
        _windows[key] = torch.from_numpy(np.hanning(2 * int(n)).astype(np.float32)).to(device) if n > 0 else torch.zeros(1, device=device)
    return _windows[key]


def _fade(device):
    import torch
    key = ("fade", str(device))
    if key not in _windows:
        _windows[key] = torch.from_numpy(np.linspace(1.0, 0.0, TAIL_FADE_SAMPLES).astype(np.float32)).to(device)
    return _windows[key]


# ---- the format ---------------------------------------------------------------------------------------------------------------------------
class AudioFormat:
    """What a request wants delivered.  `sample_rate`: any rate whose table from 22050 Hz fits 1 MiB (8000, 11025, 16000, 22050, 24000, 32000,
    44100, 48000 among them); `encoding`: pcm_s16le (int16), mulaw / alaw (G.711, uint8), pcm_f32le (float32); `gain_db`: a fixed gain;
    `peak_dbfs`: scale the whole request so its peak lands there (needs the whole request: streams refuse it); `loudness_lufs`: scale the whole
    request to that integrated loudness (ITU-R BS.1770-4, measured at the delivery rate; in [-70, 0]; not with `gain_db`; streams refuse it) --
    `peak_dbfs` given with it is a CEILING the sample peak is never raised above; `limit_dbfs`: a look-ahead limiter (5 ms) behind the gain
    holds every sample at or under that level (finite, <= 0; it replaces the static ceiling: not with `peak_dbfs`; streams take it);
    `true_peak`: `peak_dbfs` / `limit_dbfs` speak of the true peak (dBTP: the 4x oversampled signal) instead of the sample peak.  Immutable and
    hashable."""
    __slots__ = ("sample_rate", "encoding", "gain_db", "peak_dbfs", "loudness_lufs", "limit_dbfs", "true_peak")

    def __init__(self, sample_rate=SOURCE_RATE, encoding="pcm_s16le", gain_db=0.0, peak_dbfs=None, loudness_lufs=None, limit_dbfs=None,
                 true_peak=False):
        if isinstance(sample_rate, bool) or not isinstance(sample_rate, (int, np.integer)) or int(sample_rate) < 1:
            raise ValueError(f"audio_format: sample_rate must be a positive integer, got {sample_rate!r}")
        if encoding not in ENCODINGS:
            raise ValueError(f"audio_format: encoding must be one of {sorted(ENCODINGS)}, got {encoding!r}")
        if not rate_supported(SOURCE_RATE, int(sample_rate)):
            raise ValueError(f"audio_format: sample_rate {sample_rate} is not supported (its resampling table from {SOURCE_RATE} Hz exceeds "
                             f"{TABLE_MAX_BYTES} bytes)")
        try:
            gain_db = float(gain_db)
            peak_dbfs = None if peak_dbfs is None else float(peak_dbfs)
        except (TypeError, ValueError):
            raise ValueError(f"audio_format: gain_db / peak_dbfs must be numbers, got {gain_db!r} / {peak_dbfs!r}") from None
        if not math.isfinite(gain_db) or (peak_dbfs is not None and not math.isfinite(peak_dbfs)):
            raise ValueError("audio_format: gain_db / peak_dbfs must be finite")
        if peak_dbfs is not None and peak_dbfs > 0.0:
            raise ValueError(f"audio_format: peak_dbfs must be <= 0 (full scale), got {peak_dbfs}")
        if peak_dbfs is not None and gain_db != 0.0:
            raise ValueError("audio_format: give gain_db or peak_dbfs, not both")
        if loudness_lufs is not None:
            try:
                loudness_lufs = float(loudness_lufs)
            except (TypeError, ValueError):
                raise ValueError(f"audio_format: loudness_lufs must be a number, got {loudness_lufs!r}") from None
            if not (math.isfinite(loudness_lufs) and LOUDNESS_MIN_LUFS <= loudness_lufs <= 0.0):
                raise ValueError(f"audio_format: loudness_lufs must be finite and in [{LOUDNESS_MIN_LUFS:g}, 0], got {loudness_lufs}")
            if gain_db != 0.0:
                raise ValueError("audio_format: give gain_db or loudness_lufs, not both")
            if not LOUDNESS_MIN_RATE <= int(sample_rate) <= LOUDNESS_MAX_RATE:
                raise ValueError(f"audio_format: loudness_lufs needs a sample_rate in [{LOUDNESS_MIN_RATE}, {LOUDNESS_MAX_RATE}], got {sample_rate}")
        if not isinstance(true_peak, (bool, np.bool_)):
            raise ValueError(f"audio_format: true_peak must be a bool, got {true_peak!r}")
        true_peak = bool(true_peak)
        if limit_dbfs is not None:
            try:
                limit_dbfs = float(limit_dbfs)
            except (TypeError, ValueError):
                raise ValueError(f"audio_format: limit_dbfs must be a number, got {limit_dbfs!r}") from None
            if not math.isfinite(limit_dbfs) or limit_dbfs > 0.0:
                raise ValueError(f"audio_format: limit_dbfs must be finite and <= 0 (full scale), got {limit_dbfs}")
            if peak_dbfs is not None:
                raise ValueError("audio_format: give limit_dbfs or peak_dbfs, not both (the limiter replaces the static ceiling)")
            if not 1 <= limiter_lookahead(int(sample_rate)) <= LIMITER_MAX_LOOKAHEAD:
                raise ValueError(f"audio_format: limit_dbfs needs a look-ahead of 1 .. {LIMITER_MAX_LOOKAHEAD} samples; at sample_rate "
                                 f"{sample_rate} it is {limiter_lookahead(int(sample_rate))}")
        if true_peak and peak_dbfs is None and limit_dbfs is None:
            raise ValueError("audio_format: true_peak needs peak_dbfs or limit_dbfs (it says which peak they speak of)")
        for k, v in (("sample_rate", int(sample_rate)), ("encoding", encoding), ("gain_db", gain_db), ("peak_dbfs", peak_dbfs),
                     ("loudness_lufs", loudness_lufs), ("limit_dbfs", limit_dbfs), ("true_peak", true_peak)):
            object.__setattr__(self, k, v)

    def __setattr__(self, k, v):
        raise AttributeError("AudioFormat is immutable")

    def _key(self):
        base = (self.sample_rate, self.encoding, self.gain_db, self.peak_dbfs, self.loudness_lufs)
        return base if self.limit_dbfs is None and not self.true_peak else base + (self.limit_dbfs, self.true_peak)

    def key(self):
        """what equality and the hash go by: (sample_rate, encoding, gain_db, peak_dbfs, loudness_lufs), followed by (limit_dbfs, true_peak)
        when either is set"""
        return self._key()

    def __eq__(self, other):
        return isinstance(other, AudioFormat) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        loud = "" if self.loudness_lufs is None else f", loudness_lufs={self.loudness_lufs}"
        loud += "" if self.limit_dbfs is None else f", limit_dbfs={self.limit_dbfs}"
        loud += ", true_peak=True" if self.true_peak else ""
        return f"AudioFormat(sample_rate={self.sample_rate}, encoding={self.encoding!r}, gain_db={self.gain_db}, peak_dbfs={self.peak_dbfs}{loud})"

    @property
    def dtype(self):
        return DTYPES[self.encoding]

    @property
    def gain(self) -> np.float32:
        """f32(10^(dB / 20)) of gain_db, or of peak_dbfs (then divided by the measured peak on the device; under `loudness_lufs` the ceiling)"""
        return np.float32(10.0 ** ((self.gain_db if self.peak_dbfs is None else self.peak_dbfs) / 20.0))

    @property
    def ceiling(self) -> Optional[np.float32]:
        """c = f32(10^(limit_dbfs / 20)), what the limiter holds every sample under; None without a limiter"""
        return None if self.limit_dbfs is None else np.float32(10.0 ** (self.limit_dbfs / 20.0))

    @staticmethod
    def parse(value) -> Optional["AudioFormat"]:
        """None | AudioFormat | dict of the constructor's arguments | "rate/encoding", "rate" or "encoding", each optionally followed by a
        loudness target as "/-16lufs", a limiter as "/-1limit" and "/tp" for true peak ("48000/pcm_s16le/-16lufs/-1limit/tp"; up to five parts,
        in any order) -> AudioFormat (None stays None)"""
        if value is None or isinstance(value, AudioFormat):
            return value
        if isinstance(value, dict):
            extra = set(value) - set(AudioFormat.__slots__)
            if extra:
                raise ValueError(f"audio_format: unknown keys {sorted(extra)}")
            return AudioFormat(**value)
        if isinstance(value, str):
            parts = [p.strip() for p in value.split("/")]
            if not 1 <= len(parts) <= 5 or not all(parts):
                raise ValueError(f"audio_format: expected 'rate/encoding', got {value!r}")
            kw = {}
            for p in parts:
                loud, lim = _LUFS_PART.match(p), _LIMIT_PART.match(p)
                key = ("loudness_lufs" if loud else "limit_dbfs" if lim else "true_peak" if p.lower() == "tp" else
                       "sample_rate" if p.isdigit() else "encoding")
                if key in kw:
                    raise ValueError(f"audio_format: expected 'rate/encoding', got {value!r}")
                kw[key] = (float(loud.group(1)) if loud else float(lim.group(1)) if lim else True if key == "true_peak" else
                           int(p) if p.isdigit() else p)
            return AudioFormat(**kw)
        raise ValueError(f"audio_format: expected an AudioFormat, a dict or a string, got {type(value).__name__}")


def refuse_audio_format(kwargs: dict, who: str) -> None:
    """entries that deliver (22050, int16) only: a given `audio_format` is an error before any work"""
    if kwargs.get("audio_format") is not None:
        raise ValueError(f"{who}: `audio_format` is not available here (use infer_batch, infer_requests, infer_stream or stream_session of the "
                         "IndexTTS-2.5 pipeline, on one process)")


# ---- launches -------------------------------------------------------------------------------------------------------------------------------
def _dev_table(rows, device):
    import torch
    return torch.from_numpy(np.asarray(rows, dtype=np.int64).reshape(len(rows), -1)).to(device)


def gather_pieces(tails, audio, piece_total: int, keep_total: int, jobs, windows: Sequence[int], device):
    """one itts_pcm_stream_piece_seq_forward launch.  tails / audio: flat f32 device buffers (None: unused); jobs: rows of 12 ints as the header
    lists them, `win_off` counted within the concatenation of np.hanning(2n) for n in `windows`.  -> (piece buffer, keep buffer)"""
    import torch
    from . import _lib
    piece = torch.empty(max(int(piece_total), 1), dtype=torch.float32, device=device)
    keep = torch.empty(max(int(keep_total), 1), dtype=torch.float32, device=device)
    if not jobs:
        return piece, keep
    win = torch.cat([_window(n, device) for n in windows]) if windows else _window(0, device)
    table = _dev_table(jobs, device)
    longest = max(int(j[5]) + int(j[6]) for j in jobs)
    tails, audio = (t if t is not None and t.numel() else piece for t in (tails, audio))       # an empty source is never read: any valid address
    with _lib.on_device(device):
        _lib.check(_lib.lib().itts_pcm_stream_piece_seq_forward(
            _lib.ptr(tails), _lib.ptr(audio), _lib.ptr(piece), _lib.ptr(keep), _lib.ptr(win), _lib.ptr(_fade(device)), _lib.ptr(table),
            len(jobs), longest, _lib.stream_ptr(device)), "pcm_stream_piece_seq")
    return piece, keep


def resample_seq(x, seqs, orig: int, new: int, y_total: int):
    """one itts_pcm_resample_seq_forward launch.  x: flat f32 device buffer; seqs: rows (x_start, n_buf, in_offset, y_start, out_offset, n_out, final)"""
    import torch
    from . import _lib
    L, M, H, K = resample_params(orig, new)
    table = resample_table(orig, new, x.device)
    y = torch.empty(max(int(y_total), 1), dtype=torch.float32, device=x.device)
    rows = [tuple(int(v) for v in s) + (0,) for s in seqs]
    for x_start, n_buf, in_off, y_start, out_off, n_out, final, _ in rows:
        if min(x_start, n_buf, in_off, y_start, out_off, n_out) < 0 or x_start + n_buf > x.numel() or y_start + n_out > y.numel():
            raise ValueError("resample_seq: a sequence lies outside its buffer")
        if n_out > outputs_ready(in_off + n_buf, bool(final), L, M, H) - out_off:
            raise ValueError("resample_seq: a sequence asks for outputs whose support has not arrived")
        if n_out and first_needed(out_off, in_off + n_buf, L, M, H) < in_off:
            raise ValueError("resample_seq: a sequence's buffer starts after the first sample its outputs need")
    longest = max(r[5] for r in rows)
    if longest > 0:
        with _lib.on_device(x.device):
            _lib.check(_lib.lib().itts_pcm_resample_seq_forward(_lib.ptr(x), _lib.ptr(y), _lib.ptr(table), _lib.ptr(_dev_table(rows, x.device)),
                                                                len(rows), longest, L, M, H, K, _lib.stream_ptr(x.device)), "pcm_resample_seq")
    return y


def peak_seq(x, seqs):
    """per-sequence max |x| (NaN ignored) -> f32 device tensor [n_seq]; seqs: rows (x_start, n)"""
    import torch
    from . import _lib
    rows = [(int(a), int(n)) for a, n in seqs]
    if any(a < 0 or n < 0 or a + n > x.numel() for a, n in rows):
        raise ValueError("peak_seq: a sequence lies outside its buffer")
    peak = torch.empty(len(rows), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().itts_pcm_peak_seq_forward(_lib.ptr(x), _lib.ptr(peak), _lib.ptr(_dev_table(rows, x.device)), len(rows),
                                                        max(n for _, n in rows), _lib.stream_ptr(x.device)), "pcm_peak_seq")
    return peak


def true_peak_seq(x, seqs):
    """per-sequence true peak: max |u| over the sequence oversampled 1 -> 4 by the resampler (NaN ignored; the bits of `peak_seq` over
    `resample_seq(x, 1 -> 4)`, which is never written) -> f32 device tensor [n_seq]; seqs: rows (x_start, n)"""
    import torch
    from . import _lib
    rows = [(int(a), int(n)) for a, n in seqs]
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous():
        raise ValueError("true_peak_seq: x must be a flat contiguous f32 tensor")
    if not rows or any(a < 0 or n < 0 or a + n > x.numel() for a, n in rows):
        raise ValueError("true_peak_seq: a sequence lies outside its buffer")
    peak = torch.empty(len(rows), dtype=torch.float32, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().itts_pcm_truepeak_seq_forward(_lib.ptr(x), _lib.ptr(peak), _lib.ptr(resample_table(1, 4, x.device)),
                                                            _lib.ptr(_dev_table(rows, x.device)), len(rows), max(n for _, n in rows),
                                                            _lib.stream_ptr(x.device)), "pcm_truepeak_seq")
    return peak


def measure_true_peak(wave, device=None) -> float:
    """true peak in dBTP of one mono signal (ITU-R BS.1770 Annex 2 with this project's 4x prototype) as a Python float, -inf for silence.  wave:
    a host array or a device tensor; a host array is measured on `device` (default: the current one)."""
    import torch
    if torch.is_tensor(wave):
        x = wave.reshape(-1).float().contiguous()
        if device is not None:
            x = x.to(device)
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(wave, dtype=np.float32).reshape(-1))).to(device if device is not None else "cuda")
    if not x.is_cuda:
        raise ValueError("measure_true_peak: the measurement runs on the device (pass device=, or a device tensor)")
    peak = float(true_peak_seq(x, [(0, int(x.numel()))]).cpu()[0]) if x.numel() else 0.0
    return 20.0 * math.log10(peak) if peak > 0.0 else float("-inf")


def limiter_seq(x, seqs, rate: int, gain, limit_dbfs: float, true_peak: bool, y_total: int, stats: bool = False):
    """one itts_pcm_limiter_seq_forward launch.  x: flat f32 device buffer at `rate`; seqs: the resampler's rows (x_start, n_buf, in_offset,
    y_start, out_offset, n_out, final); gain: the static gain g0, an f32 device tensor [n_seq] or a scalar.  -> z, or (z, f32 [n_seq, 2] of
    min G and max |z|) with `stats`."""
    import torch
    from . import _lib
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous():
        raise ValueError("limiter_seq: x must be a flat contiguous f32 tensor")
    limit_dbfs = float(limit_dbfs)
    if not math.isfinite(limit_dbfs) or limit_dbfs > 0.0:
        raise ValueError(f"limiter_seq: limit_dbfs must be finite and <= 0, got {limit_dbfs}")
    window = limiter_window(rate, x.device)
    La, R = limiter_lookahead(rate), limiter_reach(rate, true_peak)
    z = torch.empty(max(int(y_total), 1), dtype=torch.float32, device=x.device)
    rows = [tuple(int(v) for v in s) + (0,) for s in seqs]
    if not rows:
        raise ValueError("limiter_seq: no sequence")
    for x_start, n_buf, in_off, y_start, out_off, n_out, final, _ in rows:
        if min(x_start, n_buf, in_off, y_start, out_off, n_out) < 0 or x_start + n_buf > x.numel() or y_start + n_out > z.numel():
            raise ValueError("limiter_seq: a sequence lies outside its buffer")
        if n_out > limiter_ready(in_off + n_buf, bool(final), R) - out_off:
            raise ValueError("limiter_seq: a sequence asks for outputs whose look-ahead has not arrived")
        if n_out and min(limiter_first_needed(out_off, R), in_off + n_buf) < in_off:
            raise ValueError("limiter_seq: a sequence's buffer starts after the first sample its outputs need")
    if torch.is_tensor(gain):
        if gain.dtype != torch.float32 or int(gain.numel()) != len(rows):
            raise ValueError("limiter_seq: gain must be an f32 tensor with one value per sequence")
        gain = gain.contiguous()
    else:
        gain = torch.full((len(rows),), float(np.float32(gain)), dtype=torch.float32, device=x.device)
    st = torch.empty((len(rows), 2), dtype=torch.float32, device=x.device) if stats else None
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().itts_pcm_limiter_seq_forward(
            _lib.ptr(x), _lib.ptr(z), _lib.ptr(window), _lib.ptr(resample_table(1, 4, x.device) if true_peak else None),
            _lib.ptr(_dev_table(rows, x.device)), len(rows), max(r[5] for r in rows), La, _lib.ptr(gain),
            float(np.float32(10.0 ** (limit_dbfs / 20.0))), _lib.ptr(st), _lib.stream_ptr(x.device)), "pcm_limiter_seq")
    return (z, st) if stats else z


def loudness_hop(rate: int) -> int:
    """samples of one 100 ms sub-block at `rate`: (rate + 5) // 10"""
    return (int(rate) + 5) // 10


def loudness_coefficients(rate: int) -> np.ndarray:
    """the 23 doubles of itts_pcm_loudness_coefficients: K-weighting at `rate` (stage 1 b0 b1 b2 a1 a2, stage 2 a1 a2) and the 4 x 4 hop-step
    transition of the output state, as the measuring entry builds them (host arithmetic: no device is touched)"""
    import ctypes
    from . import _lib
    out = (ctypes.c_double * 23)()
    _lib.check(_lib.lib().itts_pcm_loudness_coefficients(int(rate), out), "pcm_loudness_coefficients")
    return np.array(out, dtype=np.float64)


def _measure_seq(x, seqs, rate: int, want_peak: bool, who: str):
    """one itts_pcm_loudness_seq_forward call (four launches) -> (f64 LUFS [n_seq], f32 peak [n_seq] or None), device tensors"""
    import torch
    from . import _lib
    rate = int(rate)
    if not LOUDNESS_MIN_RATE <= rate <= LOUDNESS_MAX_RATE:
        raise ValueError(f"{who}: the rate must lie in [{LOUDNESS_MIN_RATE}, {LOUDNESS_MAX_RATE}], got {rate}")
    if x.dtype != torch.float32 or x.dim() != 1 or not x.is_contiguous():
        raise ValueError(f"{who}: x must be a flat contiguous f32 tensor")
    rows = [(int(a), int(n)) for a, n in seqs]
    if not rows or any(a < 0 or n < 0 or a + n > x.numel() for a, n in rows):
        raise ValueError(f"{who}: a sequence lies outside its buffer")
    hop, table, total = loudness_hop(rate), [], 0
    for a, n in rows:                                              # a sequence's sub-blocks own consecutive workspace rows
        table.append((a, n, total, 0))
        total += n // hop
    lufs = torch.empty(len(rows), dtype=torch.float64, device=x.device)
    peak = torch.empty(len(rows), dtype=torch.float32, device=x.device) if want_peak else None
    work = torch.empty(max(total, 1) * LOUDNESS_WS_DOUBLES, dtype=torch.float64, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().itts_pcm_loudness_seq_forward(_lib.ptr(x), _lib.ptr(lufs), _lib.ptr(peak), _lib.ptr(_dev_table(table, x.device)),
                                                            len(rows), max(n for _, n in rows), rate, total, _lib.ptr(work), work.numel() * 8,
                                                            _lib.stream_ptr(x.device)), "pcm_loudness_seq")
    return lufs, peak


def loudness_seq(x, seqs, rate: int):
    """per-sequence integrated loudness (ITU-R BS.1770-4, mono) of x sampled at `rate` -> f64 device tensor [n_seq] in LUFS,
    -inf where nothing is measurable (under 400 ms, or nothing through the gates); seqs: rows (x_start, n).  A sequence's result has the same
    bits alone, in any batch and anywhere in x."""
    return _measure_seq(x, seqs, rate, False, "loudness_seq")[0]


def loudness_gain(lufs, target_lufs: float, peak=None, ceiling_dbfs: Optional[float] = None, report: bool = False):
    """one itts_pcm_loudness_gain_forward launch: f32 gain [n_seq] = f32(10^((target - L) / 20)), 1 where L is -inf, and with `ceiling_dbfs` (needs
    `peak`) at most f32(10^(ceiling / 20)) / peak.  report: -> (gain, f64 [n_seq, 3] of L, the gain in dB, the delivered peak in dBFS)"""
    import torch
    from . import _lib
    n = int(lufs.numel())
    if lufs.dtype != torch.float64 or n < 1 or (peak is not None and (peak.dtype != torch.float32 or int(peak.numel()) != n)):
        raise ValueError("loudness_gain: lufs must be a non-empty f64 tensor and peak an f32 tensor of its length")
    if ceiling_dbfs is not None and peak is None:
        raise ValueError("loudness_gain: a ceiling needs the measured peaks")
    gain = torch.empty(n, dtype=torch.float32, device=lufs.device)
    rep = torch.empty((n, 3), dtype=torch.float64, device=lufs.device) if report else None
    with _lib.on_device(lufs.device):
        _lib.check(_lib.lib().itts_pcm_loudness_gain_forward(_lib.ptr(lufs.contiguous()), _lib.ptr(peak), _lib.ptr(gain), _lib.ptr(rep), n,
                                                             float(target_lufs), int(ceiling_dbfs is not None), float(ceiling_dbfs or 0.0),
                                                             _lib.stream_ptr(lufs.device)), "pcm_loudness_gain")
    return (gain, rep) if report else gain


def measure_loudness(wave, rate: int, device=None) -> float:
    """integrated loudness in LUFS of one mono signal -- a voice prompt, a rendered request -- as a Python float (-inf: not measurable).  wave:
    a host array or a device tensor of samples in [-1, 1]; a host array is measured on `device` (default: the current one)."""
    import torch
    if torch.is_tensor(wave):
        x = wave.reshape(-1).float().contiguous()
        if device is not None:
            x = x.to(device)
    else:
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(wave, dtype=np.float32).reshape(-1))).to(device if device is not None else "cuda")
    if not x.is_cuda:
        raise ValueError("measure_loudness: the measurement runs on the device (pass device=, or a device tensor)")
    if x.numel() == 0:
        return float("-inf")
    return float(loudness_seq(x, [(0, int(x.numel()))], rate).cpu()[0])


def encode_seq(x, seqs, encoding: str, gain, peak=None, y_total: Optional[int] = None):
    """gain and encoding -> device tensor of the encoding's dtype; seqs: rows (x_start, n, y_start); gain: f32 device tensor [n_seq] or a scalar"""
    import torch
    from . import _lib
    rows = [(int(a), int(n), int(b), 0) for a, n, b in seqs]
    total = int(y_total) if y_total is not None else max(b + n for _, n, b, _ in rows)
    if any(min(a, n, b) < 0 or a + n > x.numel() or b + n > total for a, n, b, _ in rows):
        raise ValueError("encode_seq: a sequence lies outside its buffer")
    if not torch.is_tensor(gain):
        gain = torch.full((len(rows),), float(np.float32(gain)), dtype=torch.float32, device=x.device)
    y = torch.empty(max(total, 1), dtype=torch.from_numpy(np.zeros(0, DTYPES[encoding])).dtype, device=x.device)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().itts_pcm_encode_seq_forward(_lib.ptr(x), _lib.ptr(y), _lib.ptr(_dev_table(rows, x.device)), len(rows),
                                                          max(r[1] for r in rows), ENCODINGS[encoding], _lib.ptr(gain), _lib.ptr(peak),
                                                          _lib.stream_ptr(x.device)), "pcm_encode_seq")
    return y[:total]


# ---- whole requests -------------------------------------------------------------------------------------------------------------------------
def convert(rows, lens, groups, fmt, interval_silence=200, report: Optional[list] = None,
            limiter_report: Optional[list] = None) -> List[np.ndarray]:
    """Deliver whole requests.  rows: f32 device tensor (N, T) of 22.05 kHz samples in [-1, 1] (or a list of 1-D tensors), row i valid up to
    lens[i]; groups: per request the indices of its rows, in order; fmt: AudioFormat (or what `AudioFormat.parse` takes).  Each request is
    assembled on the device -- its rows with int(22050 * interval_silence / 1000) zeros between them -- resampled as ONE sequence, its peak
    measured when the format asks, and encoded; the results come back in one device-to-host copy.  -> one 1-D array per request.
    With `loudness_lufs` the resampled sequence is measured (four launches, which also yield its peak), one launch forms the gain
    f32(10^((target - L) / 20)) -- capped at f32(10^(peak_dbfs / 20)) / peak when the format gives a ceiling -- and the encoder applies it.
    report: a list that receives, per request, dict(measured_lufs, gain_db, peak_dbfs_after) (one more small copy), or None when the format
    names no loudness (`measured_lufs` is the measurement BEFORE any limiting; the limited signal is not measured again).
    With `true_peak` the peak that `peak_dbfs` scales to (or, under loudness, caps at) is the true peak: one launch of the 4x meter.  With
    `limit_dbfs` ONE limiter launch stands between gain formation and the encoder: the loudness gain array (or the scalar gain) is its static
    gain and the encoder runs with gain 1.  limiter_report: a list that receives, per request, dict(max_reduction_db, peak_dbfs_after) -- the
    deepest gain reduction in dB (>= 0) and the delivered peak, the true peak under `true_peak` (one more small copy) -- or None."""
    import torch
    fmt = AudioFormat.parse(fmt) or AudioFormat()
    if isinstance(rows, (list, tuple)):
        lens = [int(r.numel()) for r in rows] if lens is None else lens
        width = max(max(int(r.numel()) for r in rows), 1)
        flat = torch.cat([torch.nn.functional.pad(r.reshape(-1).float(), (0, width - int(r.numel()))) for r in rows])
    else:
        rows = rows.reshape(rows.shape[0], -1)
        width = int(rows.shape[1])
        flat = rows.float().contiguous().reshape(-1)
    lens = [int(v) for v in lens]
    if any(n < 0 or n > width for n in lens):
        raise ValueError("convert: a row's length lies outside its row")
    if not groups:
        return []
    sil = int(SOURCE_RATE * interval_silence / 1000.0) if interval_silence > 0 else 0
    # assemble: a ragged copy of every segment to its place in a zeroed buffer (the piece kernel with nothing to blend)
    jobs, starts, totals, pos = [], [], [], 0
    for g in groups:
        starts.append(pos)
        for k, i in enumerate(g):
            jobs.append((0, i * width, pos, 0, 0, lens[i], 0, 0, 0, 0, 0, 0))
            pos += lens[i] + (sil if k < len(g) - 1 else 0)
        totals.append(pos - starts[-1])
    if all(len(g) == 1 for g in groups):
        src, starts = flat, [g[0] * width for g in groups]         # nothing to assemble: the rows are the requests
    else:
        src = torch.zeros(max(pos, 1), dtype=torch.float32, device=flat.device)
        _gather_into(src, flat, jobs)
    L, M, H, _ = resample_params(SOURCE_RATE, fmt.sample_rate)
    if fmt.sample_rate != SOURCE_RATE:
        outs = [resampled_length(n, L, M) for n in totals]
        y_starts = np.concatenate([[0], np.cumsum(outs)]).astype(np.int64)
        src = resample_seq(src, [(a, n, 0, int(b), 0, o, 1) for a, n, b, o in zip(starts, totals, y_starts, outs)], SOURCE_RATE, fmt.sample_rate,
                           int(y_starts[-1]))
        starts, totals = [int(v) for v in y_starts[:-1]], outs
    o_starts = np.concatenate([[0], np.cumsum(totals)]).astype(np.int64)
    rep = None
    if fmt.loudness_lufs is not None:
        # measured on what is encoded -- the request at the delivery rate -- and turned into the encoder's gain on the device: nothing waits
        # for the host between measuring and encoding.  The peak comes out of the measuring pass, so a ceiling costs no launch.
        lufs, peak = _measure_seq(src, list(zip(starts, totals)), fmt.sample_rate, True, "convert")
        if fmt.true_peak and fmt.peak_dbfs is not None:           # the ceiling speaks of the true peak: the measuring pass's sample peak is not used
            peak = true_peak_seq(src, list(zip(starts, totals)))
        gain, rep = loudness_gain(lufs, fmt.loudness_lufs, peak, fmt.peak_dbfs, report=True)
        peak = None
    else:
        peak = None
        if fmt.peak_dbfs is not None:
            peak = (true_peak_seq if fmt.true_peak else peak_seq)(src, list(zip(starts, totals)))
        gain = fmt.gain
    lim = None
    if fmt.limit_dbfs is not None:
        # every output sample is a function of its own request's samples within the limiter's reach: the request gets the audio it gets alone
        src, lim = limiter_seq(src, [(a, n, 0, int(b), 0, n, 1) for a, n, b in zip(starts, totals, o_starts)], fmt.sample_rate, gain,
                               fmt.limit_dbfs, fmt.true_peak, int(o_starts[-1]), stats=True)
        starts, gain = [int(v) for v in o_starts[:-1]], np.float32(1.0)
        if limiter_report is not None and fmt.true_peak:
            lim = torch.stack([lim[:, 0], true_peak_seq(src, list(zip(starts, totals)))], dim=1)
    enc = encode_seq(src, [(a, n, int(b)) for a, n, b in zip(starts, totals, o_starts)], fmt.encoding, gain, peak, int(o_starts[-1]))
    host = enc.cpu().numpy()                                       # the one device-to-host copy
    if report is not None:
        if rep is None:
            report.extend([None] * len(groups))
        else:                                                      # one small copy per format: three doubles per request
            report.extend(dict(measured_lufs=float(L), gain_db=float(g), peak_dbfs_after=float(p)) for L, g, p in rep.cpu().tolist())
    if limiter_report is not None:
        if lim is None:
            limiter_report.extend([None] * len(groups))
        else:                                                      # one small copy per format: two floats per request
            limiter_report.extend(dict(max_reduction_db=0.0 - 20.0 * math.log10(g) if g > 0.0 else float("inf"),
                                       peak_dbfs_after=20.0 * math.log10(p) if p > 0.0 else float("-inf")) for g, p in lim.cpu().tolist())
    return [host[int(o_starts[r]): int(o_starts[r + 1])] for r in range(len(groups))]


def _gather_into(dst, audio, jobs):
    from . import _lib
    table = _dev_table(jobs, audio.device)
    longest = max(int(j[5]) for j in jobs)
    if longest == 0:
        return
    with _lib.on_device(audio.device):
        _lib.check(_lib.lib().itts_pcm_stream_piece_seq_forward(_lib.ptr(audio), _lib.ptr(audio), _lib.ptr(dst), _lib.ptr(dst),
                                                                _lib.ptr(_window(0, audio.device)), _lib.ptr(_fade(audio.device)), _lib.ptr(table),
                                                                len(jobs), longest, _lib.stream_ptr(audio.device)), "pcm_stream_piece_seq")


# ---- streams --------------------------------------------------------------------------------------------------------------------------------
def piece_plan(tail_len: Optional[int], audio_len: int, ovlp: int, last: bool):
    """The lengths of `RowStream.push` as integers.  tail_len: None on the row's first chunk.  -> dict(n_blend, piece_len, keep_len, rest_src,
    keep_src, fade): piece = blend(tail, audio[:n_blend]) | audio[rest_src : rest_src + piece_len - n_blend], keep = audio[keep_src :
    keep_src + keep_len].  A chunk shorter than the overlap holds nothing back beyond itself (lengths clamp at 0)."""
    a, ovlp = int(audio_len), int(ovlp)
    if tail_len is None:
        n_blend, rest_src, rest_len = 0, 0, a
    else:
        n_blend, rest_src, rest_len = min(int(tail_len), min(ovlp, a)), min(ovlp, a), max(a - ovlp, 0)
    keep_len = 0 if last else min(ovlp, rest_len)
    piece_len = n_blend + rest_len - keep_len
    return dict(n_blend=n_blend, piece_len=piece_len, keep_len=keep_len, rest_src=rest_src, keep_src=rest_src + rest_len - keep_len,
                fade=bool(last) and piece_len > TAIL_FADE_SAMPLES)


def stream_format(fmt, who: str) -> Optional[AudioFormat]:
    """a stream's format: `peak_dbfs` and `loudness_lufs` need the whole request before the first sample can leave, so streams refuse them;
    `limit_dbfs` (with or without `true_peak`) is causal with a bounded delay, so a stream may have it"""
    fmt = AudioFormat.parse(fmt)
    if fmt is not None and fmt.peak_dbfs is not None:
        raise ValueError(f"{who}: audio_format with peak_dbfs needs the whole request; a stream cannot deliver it (use gain_db, or infer_requests)")
    if fmt is not None and fmt.loudness_lufs is not None:
        raise ValueError(f"{who}: audio_format with loudness_lufs needs the whole request; a stream cannot deliver it (use gain_db, or "
                         "infer_requests)")
    return fmt


class OutputStream:
    """What one stream carries between renders on the device: the held-back tail of the cross-fade (`RowStream.tail`), the resampler's
    history and its counters.  `deliver` advances a batch of them."""

    def __init__(self, fmt, ovlp: int):
        self.fmt = stream_format(fmt, "OutputStream") or AudioFormat()
        self.ovlp = int(ovlp)
        self.params = resample_params(SOURCE_RATE, self.fmt.sample_rate)
        self.tail = None              # f32 device tensor: samples waiting for the next chunk's head
        self.started = self.finished = False
        self.carry = None             # f32 device tensor: the stream's samples n_in - len(carry) .. n_in
        self.n_in = self.n_out = 0    # samples received / outputs produced so far
        self.lim_carry = None         # f32 device tensor: the limiter's input (delivery rate) from lim_out - R onward
        self.lim_in = self.lim_out = 0                             # delivery-rate samples the limiter has received / produced

    @property
    def sample_rate(self) -> int:
        return self.fmt.sample_rate


def deliver(streams: Sequence[OutputStream], audios: Sequence, lasts: Sequence[bool]) -> List[Optional[np.ndarray]]:
    """The device form of `RowStream.push` (audios[i]: the chunk's f32 device row) and `RowStream.flush` (audios[i] None) for all jobs of a
    render: ONE piece launch, per format ONE resample launch, ONE encode launch and ONE device-to-host copy.  A stream may appear once per
    call.  -> the encoded pieces (None for a flush with nothing held back)."""
    import torch
    n = len(streams)
    out: List[Optional[np.ndarray]] = [None] * n
    if len(set(map(id, streams))) != n:
        raise ValueError("deliver: a stream may appear once per call")
    live = [i for i in range(n) if not streams[i].finished and (audios[i] is not None or streams[i].tail is not None)]
    for i in range(n):
        if i not in live and audios[i] is None:
            streams[i].finished = True
    if not live:
        return out
    device = next(a for a in (audios[i] if audios[i] is not None else streams[i].tail for i in live)).device
    # (d) pieces
    a_list = [audios[i].reshape(-1).float() for i in live if audios[i] is not None]
    t_list = [streams[i].tail for i in live if streams[i].tail is not None]
    audio = torch.cat(a_list) if len(a_list) > 1 else (a_list[0].contiguous() if a_list else None)
    tails = torch.cat(t_list) if len(t_list) > 1 else (t_list[0].contiguous() if t_list else None)
    jobs, windows, plans = [], [], []
    a_pos = t_pos = p_pos = k_pos = w_pos = 0
    for i in live:
        s = streams[i]
        t_len = None if s.tail is None else int(s.tail.numel())
        if audios[i] is None:                                      # flush: the held-back samples, faded, end the stream
            plan = dict(n_blend=0, piece_len=t_len, keep_len=0, rest_src=0, keep_src=0, fade=t_len > TAIL_FADE_SAMPLES)
            flags, a_len, last = 2, 0, True
        else:
            a_len, last = int(audios[i].numel()), bool(lasts[i])
            plan = piece_plan(t_len, a_len, s.ovlp, last)
            flags = 0
        nb = plan["n_blend"]
        jobs.append((t_pos, a_pos, p_pos, k_pos, nb, plan["piece_len"], plan["keep_len"], plan["rest_src"], plan["keep_src"], w_pos,
                     flags | int(plan["fade"]), 0))
        plans.append((i, p_pos, plan["piece_len"], k_pos, plan["keep_len"], last))
        if nb:
            windows.append(nb)
            w_pos += 2 * nb
        a_pos, t_pos, p_pos, k_pos = a_pos + a_len, t_pos + (t_len or 0), p_pos + plan["piece_len"], k_pos + plan["keep_len"]
    piece, keep = gather_pieces(tails, audio, p_pos, k_pos, jobs, windows, device)
    for i, _, _, k0, kn, last in plans:
        s = streams[i]
        s.started, s.tail, s.finished = True, (None if last else keep[k0: k0 + kn]), last
    # (a) + (c) per format
    by_fmt = {}
    for rec in plans:
        by_fmt.setdefault(streams[rec[0]].fmt, []).append(rec)
    for fmt, recs in by_fmt.items():
        L, M, H, _ = resample_params(SOURCE_RATE, fmt.sample_rate)
        if fmt.sample_rate == SOURCE_RATE:
            src, spans = piece, [(p0, pn) for _, p0, pn, _, _, _ in recs]
        else:
            parts, seqs, x_pos, y_pos = [], [], 0, 0
            for i, p0, pn, _, _, last in recs:
                s = streams[i]
                c_len = 0 if s.carry is None else int(s.carry.numel())
                if c_len:
                    parts.append(s.carry)
                parts.append(piece[p0: p0 + pn])
                n_in = s.n_in + pn
                n_new = outputs_ready(n_in, last, L, M, H) - s.n_out
                seqs.append((x_pos, c_len + pn, s.n_in - c_len, y_pos, s.n_out, n_new, int(last)))
                x_pos, y_pos = x_pos + c_len + pn, y_pos + n_new
            x = torch.cat(parts)                                   # [carry | piece] per stream
            src = resample_seq(x, seqs, SOURCE_RATE, fmt.sample_rate, y_pos)
            spans = []
            for (i, _, pn, _, _, last), (x0, nb, in_off, y0, _, n_new, _) in zip(recs, seqs):
                s = streams[i]
                s.n_in, s.n_out = s.n_in + pn, s.n_out + n_new
                keep_from = first_needed(s.n_out, s.n_in, L, M, H)
                s.carry = None if last else x[x0 + (keep_from - in_off): x0 + nb]
                spans.append((y0, n_new))
        gain = fmt.gain
        if fmt.limit_dbfs is not None:
            # the limiter over [carry | new samples] per stream: an output leaves once its look-ahead has arrived, the final call the rest
            R = limiter_reach(fmt.sample_rate, fmt.true_peak)
            parts, seqs, x_pos, z_pos = [], [], 0, 0
            for (i, _, _, _, _, last), (y0, n_new) in zip(recs, spans):
                s = streams[i]
                c_len = 0 if s.lim_carry is None else int(s.lim_carry.numel())
                if c_len:
                    parts.append(s.lim_carry)
                parts.append(src[y0: y0 + n_new])
                n_z = limiter_ready(s.lim_in + n_new, last, R) - s.lim_out
                seqs.append((x_pos, c_len + n_new, s.lim_in - c_len, z_pos, s.lim_out, n_z, int(last)))
                x_pos, z_pos = x_pos + c_len + n_new, z_pos + n_z
            x = torch.cat(parts) if x_pos else torch.zeros(1, dtype=torch.float32, device=device)
            src = limiter_seq(x, seqs, fmt.sample_rate, gain, fmt.limit_dbfs, fmt.true_peak, z_pos)
            spans, gain = [], np.float32(1.0)
            for (i, _, _, _, _, last), (x0, nb, in_off, z0, _, n_z, _) in zip(recs, seqs):
                s = streams[i]
                s.lim_in, s.lim_out = in_off + nb, s.lim_out + n_z
                s.lim_carry = None if last else x[x0 + (limiter_first_needed(s.lim_out, R) - in_off): x0 + nb]
                spans.append((z0, n_z))
        o_starts = np.concatenate([[0], np.cumsum([m for _, m in spans])]).astype(np.int64)
        if int(o_starts[-1]) == 0:
            host = np.zeros(0, dtype=fmt.dtype)
        else:
            host = encode_seq(src, [(a, m, int(b)) for (a, m), b in zip(spans, o_starts)], fmt.encoding, gain, None,
                              int(o_starts[-1])).cpu().numpy()
        for k, rec in enumerate(recs):
            out[rec[0]] = host[int(o_starts[k]): int(o_starts[k + 1])]
    return out


# ---- files ----------------------------------------------------------------------------------------------------------------------------------
def save_audio_wav(path: str, data, fmt) -> None:
    """mono WAV of an encoded array: format tag 1 (pcm_s16le), 3 (pcm_f32le), 6 (alaw) or 7 (mulaw); the non-PCM tags get the 18-byte fmt chunk
    and a `fact` chunk with the sample count, as the WAVE specification asks."""
    fmt = AudioFormat.parse(fmt) or AudioFormat()
    data = np.ascontiguousarray(np.asarray(data).reshape(-1))
    if data.dtype != np.dtype(fmt.dtype):
        raise ValueError(f"save_audio_wav: {fmt.encoding} data is {np.dtype(fmt.dtype).name}, got {data.dtype.name}")
    tag, width = WAV_TAGS[fmt.encoding], data.dtype.itemsize
    payload = data.astype(data.dtype.newbyteorder("<"), copy=False).tobytes()
    head = struct.pack("<HHIIHH", tag, 1, fmt.sample_rate, fmt.sample_rate * width, width, 8 * width)
    chunks = b"fmt " + struct.pack("<I", len(head)) + head
    if tag != 1:
        head += struct.pack("<H", 0)
        chunks = b"fmt " + struct.pack("<I", len(head)) + head + b"fact" + struct.pack("<II", 4, data.size)
    chunks += b"data" + struct.pack("<I", len(payload)) + payload + (b"\0" if len(payload) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)
