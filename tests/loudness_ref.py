"""f64 restatement of the loudness measurement of the delivery formats (include/indextts_hip.h, "loudness normalisation"),
written from the definition: ITU-R BS.1770-4 integrated loudness of a mono signal, with the K-weighting obtained by bilinear transform so that
any rate works.  Numpy and plain loops only -- nothing of the engine is imported.

K-weighting at fs.  Stage 1 (shelf): f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, K = tan(pi f0 / fs),
Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2, b = [(Vh + Vb K/Q + K^2), 2 (K^2 - Vh), (Vh - Vb K/Q + K^2)] / a0,
a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0].  Stage 2 (high-pass): f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1], the same a.
Measurement: zero initial state, NaN counts as 0; hop = (fs + 5) // 10; S_k the sums of y^2 over the whole sub-blocks; z_j = (S_j + .. + S_j+3) /
(4 hop), l_j = -0.691 + 10 log10 z_j; keep l_j > -70, then also l_j > (-0.691 + 10 log10 mean(z over those)) - 10; L = -0.691 + 10 log10 mean(z
over the kept); -inf with fewer than four sub-blocks or nothing kept."""
import math

import numpy as np

ABS_GATE = -70.0
OFFSET = -0.691


def coefficients(fs):
    """-> (b1, a1, b2, a2), each three f64"""
    fs = float(fs)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return b1, a1, b2, a2


def hop(fs) -> int:
    return (int(fs) + 5) // 10


def _biquad(x, b, a, y_hist=(0.0, 0.0)):
    """direct form 1 from zero input history and the given output history (y[-1], y[-2])"""
    b0, b1, b2, a1, a2 = float(b[0]), float(b[1]), float(b[2]), float(a[1]), float(a[2])
    x1 = x2 = 0.0
    y1, y2 = float(y_hist[0]), float(y_hist[1])
    out = np.empty(len(x), dtype=np.float64)
    for n, x0 in enumerate(x.tolist()):
        y0 = b0 * x0 + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        out[n] = y0
        x2, x1, y2, y1 = x1, x0, y1, y0
    return out


def k_weight(x, fs):
    """the K-weighted signal in f64; a NaN sample counts as 0"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    x = np.where(np.isnan(x), 0.0, x)
    b1, a1, b2, a2 = coefficients(fs)
    return _biquad(_biquad(x, b1, a1), b2, a2)


def transition(fs):
    """the 4 x 4 map of the output state (y1[-1], y1[-2], y2[-1], y2[-2]) over hop(fs) samples of zero input, by running the filters"""
    b1, a1, b2, a2 = coefficients(fs)
    h = hop(fs)
    zero = np.zeros(h)
    phi = np.zeros((4, 4))
    for c in range(4):
        s = np.zeros(4)
        s[c] = 1.0
        y1 = _biquad(zero, b1, a1, (s[0], s[1]))
        # stage 2 sees y1 with the history (s[0], s[1]) as its INPUT history: prepend it and drop the two outputs it produces
        ext = np.concatenate([[s[1], s[0]], y1])
        b0, bb1, bb2, aa1, aa2 = b2[0], b2[1], b2[2], a2[1], a2[2]
        q1, q2 = s[2], s[3]
        for n in range(2, len(ext)):
            y0 = b0 * ext[n] + bb1 * ext[n - 1] + bb2 * ext[n - 2] - aa1 * q1 - aa2 * q2
            q2, q1 = q1, y0
        phi[:, c] = [y1[-1], y1[-2], q1, q2]
    return phi


def measure(x, fs):
    """-> dict(lufs, n_blocks, kept_abs, kept, margin, l): the integrated loudness, the number of 400 ms blocks, how many pass the absolute gate
    and both gates, the smallest distance in LU of any block's loudness to a gate it was compared with, and the block loudnesses"""
    y = k_weight(x, fs)
    h = hop(fs)
    n_sub = len(y) // h
    out = dict(lufs=-math.inf, n_blocks=max(n_sub - 3, 0), kept_abs=0, kept=0, margin=math.inf, l=np.zeros(0))
    if n_sub < 4:
        return out
    S = np.array([float(np.sum(y[k * h: (k + 1) * h] ** 2)) for k in range(n_sub)])
    z = np.array([(S[j] + S[j + 1] + S[j + 2] + S[j + 3]) / (4.0 * h) for j in range(n_sub - 3)])
    with np.errstate(divide="ignore"):
        l = OFFSET + 10.0 * np.log10(z)
    out["l"] = l
    finite = np.isfinite(l)
    margin = float(np.min(np.abs(l[finite] - ABS_GATE))) if finite.any() else math.inf
    keep = l > ABS_GATE
    out["kept_abs"] = int(keep.sum())
    if keep.any():
        rel = OFFSET + 10.0 * math.log10(float(np.mean(z[keep]))) - 10.0
        margin = min(margin, float(np.min(np.abs(l[keep] - rel))))
        keep &= l > rel
        out["kept"] = int(keep.sum())
        if keep.any():
            out["lufs"] = OFFSET + 10.0 * math.log10(float(np.mean(z[keep])))
    out["margin"] = margin
    return out


def loudness(x, fs) -> float:
    return measure(x, fs)["lufs"]


def gain(lufs, target, peak=None, ceiling_dbfs=None) -> np.float32:
    """g = f32(10^((target - L) / 20)), formed in f64 and rounded once; 1 for L = -inf; under a ceiling P and a peak p > 0 at most the f32
    quotient f32(10^(P/20)) / p"""
    g = np.float32(1.0) if lufs == -math.inf else np.float32(10.0 ** ((float(target) - float(lufs)) / 20.0))
    if ceiling_dbfs is not None and peak is not None and np.float32(peak) > 0:
        g = min(g, np.float32(np.float32(10.0 ** (float(ceiling_dbfs) / 20.0)) / np.float32(peak)))
    return np.float32(g)


def tone(freq, seconds, fs, dbfs=0.0):
    n = np.arange(int(round(seconds * fs)), dtype=np.float64)
    return (10.0 ** (dbfs / 20.0)) * np.sin(2.0 * math.pi * freq * n / fs)
