"""f64 restatements of the delivery-format kernels (include/indextts_hip.h, "delivery formats"), written from the
definitions and sharing no code with indextts_amd/output.py:

  prototype / taps      the Kaiser-windowed sinc and, per output, the (coefficient, input index) pairs of its support
  resample              y[m] = sum_i h[m*M - i*L] x[i] as a direct f64 sum over the f32-rounded prototype, with sum |h x| for the error bound
  ready / stream_split  the streaming counts: which outputs a piece may produce, which input the next one still needs
  encode_*              gain, pcm_s16le (round half to even), table-free G.711, pcm_f32le
  piece                 RowStream.push / flush on f64 with streaming.crossfade / fade_out_tail
"""
import math

import numpy as np

Z, BETA = 24, 10.0
RATES = (8000, 11025, 16000, 24000, 32000, 44100, 48000)      # what the issue names, from 22050 Hz
SPLITS = ("ones", "sevens", "prime", "random", "empty_final")


def params(orig, new):
    g = math.gcd(orig, new)
    M, L = orig // g, new // g
    fs_hi, two_fc = orig * L, min(orig, new)
    H = math.ceil(Z * fs_hi / two_fc)
    assert Z * fs_hi % two_fc != 0 or H == Z * fs_hi // two_fc
    return L, M, H, math.ceil((2 * H + 1) / L)


def prototype(orig, new):
    """h[n + H], n = -H .. H, f64"""
    L, M, H, _ = params(orig, new)
    fs_hi, two_fc = float(orig * L), float(min(orig, new))
    n = np.arange(-H, H + 1, dtype=np.float64)
    arg = two_fc * n / fs_hi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(n == 0, 1.0, np.sin(np.pi * arg) / (np.pi * arg))
    return L * (two_fc / fs_hi) * sinc * np.kaiser(2 * H + 1, BETA)


def prototype_f32(orig, new):
    """the prototype as the kernel sees it: rounded once to f32, held in f64"""
    return prototype(orig, new).astype(np.float32).astype(np.float64)


def out_len(n, L, M):
    return -(-n * L // M)


def support(m, n_in, L, M, H):
    """input indices i, ascending, with |m*M - i*L| <= H and 0 <= i < n_in"""
    lo = max(0, -((H - m * M) // L))
    hi = min(n_in - 1, (m * M + H) // L)
    return range(lo, hi + 1)


def resample(x, orig, new, h=None, outputs=None):
    """-> (y, mag): the direct sum in f64 over the f32 prototype, and sum |h x| per output.  `outputs`: an iterable of m (default: all)"""
    L, M, H, _ = params(orig, new)
    h = prototype_f32(orig, new) if h is None else h
    x = np.asarray(x, dtype=np.float64)
    ms = range(out_len(len(x), L, M)) if outputs is None else outputs
    y, mag = [], []
    for m in ms:
        idx = np.fromiter(support(m, len(x), L, M, H), dtype=np.int64)
        if idx.size == 0:
            y.append(0.0), mag.append(0.0)
            continue
        t = h[m * M - idx * L + H] * x[idx]
        y.append(float(np.sum(t))), mag.append(float(np.sum(np.abs(t))))
    return np.array(y), np.array(mag)


def ready(n_in, final, L, M, H):
    """number of outputs producible from n_in samples: all m with m*M + H < n_in*L, or all ceil(n_in*L / M) on the final call"""
    if final:
        return out_len(n_in, L, M)
    top = n_in * L - H - 1                                         # m*M <= top
    return top // M + 1 if top >= 0 else 0


def splits(kind, n, rng):
    """piece lengths summing to n"""
    if kind == "ones":
        return [1] * n
    if kind == "sevens":
        return [7] * (n // 7) + ([n % 7] if n % 7 else [])
    if kind == "prime":
        return [211] * (n // 211) + ([n % 211] if n % 211 else [])
    if kind == "empty_final":
        cut = n // 2
        return [cut, n - cut, 0]
    out, left = [], n
    while left:
        k = int(rng.integers(1, max(2, min(left, 700)) + 1))
        k = min(k, left)
        out.append(k)
        left -= k
    return out


def stream_schedule(pieces, L, M, H):
    """per piece (the last one final): (n_in after it, first output, outputs produced, earliest input the NEXT piece needs)"""
    sched, n_in, done = [], 0, 0
    for k, p in enumerate(pieces):
        n_in += p
        r = ready(n_in, k == len(pieces) - 1, L, M, H)
        need = min(max(0, -((H - r * M) // L)), n_in)
        sched.append((n_in, done, r - done, need))
        done = r
    return sched


# ---- encoders -----------------------------------------------------------------------------------------------------------------------------
def scaled(x, gain):
    """s = x * gain as the kernel forms it: ONE f32 multiply, NaN -> 0"""
    s = (np.asarray(x, dtype=np.float32) * np.float32(gain)).astype(np.float32)
    return np.where(np.isnan(s), np.float32(0), s)


def encode_s16(x, gain=1.0):
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.clip((scaled(x, gain) * np.float32(32767)).astype(np.float32), np.float32(-32767), np.float32(32767))
    return np.rint(v.astype(np.float64)).astype(np.int16)                  # np.rint rounds half to even


def encode_f32(x, gain=1.0):
    return np.clip(scaled(x, gain), np.float32(-1), np.float32(1)).astype(np.float32)


def _segment(v, first_end):
    end, seg = first_end, 0
    while seg < 8 and v > end:
        end, seg = 2 * end + 1, seg + 1
    return seg


def ulaw_of(q):
    """ITU-T G.711 mu-law of one 16-bit sample, as Sun's g711.c (and CPython's audioop) codes its top 14 bits"""
    v, mask = int(q) >> 2, 0xFF
    if v < 0:
        v, mask = -v, 0x7F
    v = min(v, 8159) + 33
    seg = _segment(v, 0x3F)
    return (0x7F ^ mask) if seg >= 8 else (((seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask)


def alaw_of(q):
    """ITU-T G.711 A-law of one 16-bit sample (its top 13 bits)"""
    v, mask = int(q) >> 3, 0xD5
    if v < 0:
        v, mask = -v - 1, 0x55
    seg = _segment(v, 0x1F)
    if seg >= 8:
        return 0x7F ^ mask
    return ((seg << 4) | ((v >> 1 if seg < 2 else v >> seg) & 0xF)) ^ mask


def g711(q, law):
    f = ulaw_of if law == "mulaw" else alaw_of
    lut = np.array([f(v) for v in range(-32768, 32768)], dtype=np.uint8)
    return lut[np.asarray(q, dtype=np.int64) + 32768]


def encode(x, encoding, gain=1.0):
    if encoding == "pcm_f32le":
        return encode_f32(x, gain)
    q = encode_s16(x, gain)
    return q if encoding == "pcm_s16le" else g711(q, encoding)


# ---- stream pieces ------------------------------------------------------------------------------------------------------------------------
def piece(tail, audio, ovlp, last):
    """RowStream.push on f64 (tail None: the row's first chunk; audio None: flush) -> (piece, new tail or None, |tail| + |head| per piece sample)
    with streaming.crossfade / fade_out_tail; a chunk shorter than the overlap holds back what it has past the overlap, never a negative slice."""
    from indextts_amd.streaming import crossfade, fade_out_tail
    if audio is None:
        t = np.asarray(tail, dtype=np.float64)
        return fade_out_tail(t), None, np.abs(t)
    a = np.asarray(audio, dtype=np.float64)
    if tail is None:
        blended, rest, mag_b = np.zeros(0), a, np.zeros(0)
    else:
        t = np.asarray(tail, dtype=np.float64)
        head = a[:ovlp]
        blended, rest = crossfade(t, head).astype(np.float64), a[ovlp:]
        n = len(blended)
        mag_b = np.abs(t[:n]) + np.abs(head[:n])
    k = 0 if last else min(ovlp, len(rest))
    out = np.concatenate([blended, rest[: len(rest) - k]])
    mag = np.concatenate([mag_b, np.abs(rest[: len(rest) - k])])
    if last:
        return fade_out_tail(out), None, mag
    return out, rest[len(rest) - k:], mag
