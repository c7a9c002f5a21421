"""f64 restatement of the look-ahead limiter and the true-peak meter (include/indextts_hip.h, "look-ahead limiter"), written
from the definitions and sharing no code with indextts_amd/output.py:

  lookahead / reach / window   La = (rate * 5 + 500) // 1000, R = La (+ 24 with true peak), w[k] ~ sin^2(pi (k + 1) / (La + 2))
  oversample / true_peak       u = the direct-sum (1 -> 4) resampler of tests/pcm_ref.py, max |u| with NaN ignored
  magnitude_*                  a[n] in sample mode and in true-peak mode, in f32 as the kernel forms them (exactly reproducible in numpy)
  limiter                      r, the look-ahead minimum, the smoothing chain and the clamp in f64
  limiter_f32                  the same in f32 with the kernel's operation order -- its bits, through an exact f32 fma
"""
from fractions import Fraction

import numpy as np

from tests import pcm_ref as R

Z = R.Z
F32 = np.float32


def lookahead(rate):
    return (rate * 5 + 500) // 1000


def reach(rate, true_peak):
    return lookahead(rate) + (Z if true_peak else 0)


def ceiling(limit_db):
    """c = f32(10^(limit / 20))"""
    return F32(10.0 ** (limit_db / 20.0))


def window(rate):
    """w[0 .. La]: normalised in f64, rounded once to f32"""
    La = lookahead(rate)
    w = np.sin(np.pi * (np.arange(La + 1, dtype=np.float64) + 1.0) / (La + 2.0)) ** 2
    return (w / np.sum(w)).astype(F32)


def ready(n_in, final, reach_):
    """brute force: the number of leading outputs n with n + R < n_in (all n_in when final)"""
    if final:
        return n_in
    k = 0
    while k + reach_ < n_in:
        k += 1
    return k


def first_needed(n_out, reach_):
    """brute force: the earliest non-negative sample index within R of output n_out"""
    i = n_out
    while i > 0 and n_out - (i - 1) <= reach_:
        i -= 1
    return i


def oversample(x):
    """-> (u, mag): u[q], 0 <= q < 4N, as the f64 direct sum over the f32 prototype of the pair (1, 4), and sum |h x| per output"""
    if len(x) == 0:
        return np.zeros(0), np.zeros(0)
    return R.resample(x, 1, 4)


def peak_of(u):
    """max |u|, NaN ignored, 0 for nothing"""
    u = np.abs(np.asarray(u, dtype=np.float64))
    u = u[~np.isnan(u)]
    return float(u.max()) if u.size else 0.0


def true_peak(x):
    return peak_of(oversample(x)[0])


def scaled(x, g0):
    """s = f32(x * g0): one f32 multiply (NaN kept)"""
    with np.errstate(invalid="ignore"):
        return (np.asarray(x, dtype=F32) * F32(g0)).astype(F32)


def magnitude_sample(x, g0):
    a = np.abs(scaled(x, g0))
    return np.where(np.isnan(a), F32(0), a).astype(F32)


def magnitude_true_peak(u, n, g0):
    """a[j] = f32(max over |p| <= 3 of |u[4j + p]| * |g0|), u = 0 outside [0, 4n), NaN ignored: an exact max, then one f32 multiply"""
    u = np.abs(np.asarray(u, dtype=F32))
    assert len(u) == 4 * n
    pad = np.concatenate([np.zeros(3, F32), u, np.zeros(3, F32)])
    best = np.zeros(n, F32)
    for p in range(7):                                             # pad[4j + p] = |u[4j + p - 3]|
        best = np.fmax(best, pad[p: p + 4 * n: 4][:n])
    return (best * np.abs(F32(g0))).astype(F32)


def window_min(r, La):
    """m[j] = min r[j .. j + La] for j = -La .. N - 1 (r = 1 outside [0, N)), returned with m[j] at index j + La"""
    n = len(r)
    ext = np.concatenate([np.ones(La, r.dtype), r, np.ones(La, r.dtype)])
    m = ext[: n + La].copy()
    for k in range(1, La + 1):
        m = np.minimum(m, ext[k: k + n + La])
    return m


def limiter(s, a, rate, limit_db):
    """the definitions in f64 over the f32 inputs s = f32(x g0) and a -> (z, G)"""
    La, c = lookahead(rate), float(ceiling(limit_db))
    s64, a64 = np.asarray(s, dtype=np.float64), np.asarray(a, dtype=np.float64)
    n = len(s64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a64 > c, c / a64, 1.0)
    m = window_min(r, La)
    w = window(rate).astype(np.float64)
    acc = np.zeros(n)
    for k in range(La + 1):                                        # m[n - k] sits at index n - k + La
        acc += w[k] * (1.0 - m[La - k: La - k + n])
    G = 1.0 - acc
    with np.errstate(invalid="ignore"):
        z = np.clip(s64 * G, -c, c)
    return np.where(np.isnan(z), 0.0, z), G


def fmaf(a, b, c):
    """f32 fma of arrays, exactly.  a * b is exact in f64; their f64 sum with c, rounded again to f32, can differ from the single rounding only
    where the f64 sum sits on an f32 tie: those elements are redone in rational arithmetic."""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = s.astype(F32)
    tie = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    for i in np.flatnonzero(tie):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        near = [out[i], np.nextafter(out[i], F32(np.inf)), np.nextafter(out[i], F32(-np.inf))]
        out[i] = min(near, key=lambda v: (abs(Fraction(float(v)) - exact), int(F32(v).view(np.uint32)) & 1))
    return out


def limiter_f32(s, a, rate, limit_db):
    """the kernel's own arithmetic: one f32 division, the exact minimum, the ascending fmaf chain from 0.f, 1.f - acc, one multiply, the clamp
    -> (z, G) in f32"""
    La, c = lookahead(rate), ceiling(limit_db)
    s, a = np.asarray(s, dtype=F32), np.asarray(a, dtype=F32)
    n = len(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(a > c, c / a, F32(1)).astype(F32)
    m = window_min(r, La)
    w = window(rate)
    acc = np.zeros(n, F32)
    for k in range(La + 1):
        acc = fmaf(np.full(n, w[k], F32), (F32(1) - m[La - k: La - k + n]).astype(F32), acc)
    G = (F32(1) - acc).astype(F32)
    with np.errstate(invalid="ignore"):
        z = (s * G).astype(F32)
    z = np.where(np.isnan(z), F32(0), z)
    return np.clip(z, -c, c).astype(F32), G
