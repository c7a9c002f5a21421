"""The limiter kernels (csrc/limiter_kernels.hip; include/indextts_hip.h, "look-ahead limiter") against the f64 restatement of
tests/limiter_ref.py: the true-peak meter against the resampler it fuses and against the direct sum, the limiter in both modes at its edges,
its statistics, and the bits it keeps alone, in any batch order and as a stream."""
import functools

import numpy as np
import pytest
import torch

from indextts_amd import _lib, output as O
from tests import limiter_ref as LM
from tests import pcm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SRC = 22050
RATES = (8000, 22050, 48000)
U = 2.0 ** -24
GUARD = 12345.0
LIMIT = -1.0
TILE = O.LIMITER_TILE
F32 = np.float32


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


@functools.lru_cache(maxsize=None)
def _signals(rate):
    """per length: noise of amplitude 0.5 with a 3x burst, impulses at index 0, at N - 1 and on the 1023 / 1024 tile boundary, one NaN sample in
    the longest; each with its own static gain.  -> [(x, g0)], never written again"""
    La = LM.lookahead(rate)
    rng = np.random.default_rng(rate)
    out = []
    for k, n in enumerate((0, 1, La, La + 1, 2 * La + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + La + 3)):
        x = rng.uniform(-0.5, 0.5, n).astype(F32)
        if n >= 16:
            x[n // 3: n // 3 + 5] *= F32(3.0)
        if n >= 1:
            x[0] = F32(1.3)
        if n >= 2:
            x[n - 1] = F32(-1.2)
        if n > TILE:
            x[TILE - 1], x[TILE] = F32(1.25), F32(-1.35)
        if n > 2 * TILE:
            x[TILE + TILE // 2] = np.nan
        x.setflags(write=False)
        out.append((x, (1.0, 1.25, 0.8)[k % 3]))
    return out


def _pack(xs, order, gap=5):
    parts, starts, pos = [np.full(gap, np.nan, F32)], {}, gap
    for i in order:
        starts[i] = pos
        parts += [xs[i], np.full(gap, np.nan, F32)]
        pos += len(xs[i]) + gap
    return _dev(np.concatenate(parts)), starts


def _limit_packed(rate, order, true_peak):
    """one launch over the sequences in `order`: NaN canaries between the packed inputs, guard values around every output -> ({i: z}, {i: stats})"""
    sig = _signals(rate)
    x, starts = _pack([s[0] for s in sig], order)
    gap, seqs, z_pos = 5, [], 5
    for i in order:
        n = len(sig[i][0])
        seqs.append((starts[i], n, 0, z_pos, 0, n, 1, 0))
        z_pos += n + gap
    z = torch.full((z_pos,), GUARD, dtype=torch.float32, device=DEV)
    stats = torch.full((len(order), 2), GUARD, dtype=torch.float32, device=DEV)
    gain = _dev([sig[i][1] for i in order])
    table4 = O.resample_table(1, 4, DEV) if true_peak else None
    _lib.check(_lib.lib().itts_pcm_limiter_seq_forward(
        _lib.ptr(x), _lib.ptr(z), _lib.ptr(O.limiter_window(rate, DEV)), _lib.ptr(table4), _lib.ptr(_dev(seqs, np.int64)), len(seqs),
        max(s[5] for s in seqs), O.limiter_lookahead(rate), _lib.ptr(gain), float(LM.ceiling(LIMIT)), _lib.ptr(stats), _lib.stream_ptr(DEV)),
        "pcm_limiter_seq")
    z, stats = z.cpu().numpy(), stats.cpu().numpy()
    outs, guards = {}, np.ones(z_pos, dtype=bool)
    for i, s in zip(order, seqs):
        outs[i] = z[s[3]: s[3] + s[5]].copy()
        guards[s[3]: s[3] + s[5]] = False
    assert np.all(z[guards] == GUARD), "a block wrote outside its sequence's output"
    return outs, {i: stats[k] for k, i in enumerate(order)}


@functools.lru_cache(maxsize=None)
def _forward(rate, true_peak):
    order = tuple(range(len(_signals(rate))))
    return _limit_packed(rate, order, true_peak)


@functools.lru_cache(maxsize=None)
def _oversampled(rate):
    """the device's own resample_seq(1 -> 4) of every sequence -> [u], f32"""
    sig = _signals(rate)
    order = list(range(len(sig)))
    x, starts = _pack([s[0] for s in sig], order)
    seqs, pos = [], 0
    for i in order:
        n = len(sig[i][0])
        seqs.append((starts[i], n, 0, pos, 0, 4 * n, 1))
        pos += 4 * n
    u = O.resample_seq(x, seqs, 1, 4, pos)
    return x, starts, [(s[3], s[5]) for s in seqs], u


def _near(a, c, La):
    """samples within La of one whose magnitude exceeds c"""
    near = np.zeros(len(a), bool)
    for i in np.flatnonzero(a > c):
        near[max(0, i - La): i + La + 1] = True
    return near


def _check_against_f64(rate, true_peak, mags):
    La, c = LM.lookahead(rate), LM.ceiling(LIMIT)
    got, _ = _forward(rate, true_peak)
    worst, untouched = 0.0, 0
    for i, (x, g0) in enumerate(_signals(rate)):
        s, a = LM.scaled(x, g0), mags[i]
        z_ref, _ = LM.limiter(s, a, rate, LIMIT)
        z = got[i]
        assert z.shape == z_ref.shape == x.shape and np.all(np.isfinite(z)), len(x)
        bound = (La + 1 + 4) * U * np.abs(np.nan_to_num(s.astype(np.float64)))
        err = np.abs(z.astype(np.float64) - z_ref)
        if len(x):
            worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (len(x), float(err.max()))
        if not true_peak:
            assert np.all(np.abs(z) <= c), len(x)                   # the ceiling, as an exact f32 compare
        quiet = ~_near(a, c, La) & ~np.isnan(s)
        untouched += int(quiet.sum())
        assert np.array_equal(z[quiet].view(np.uint32), s[quiet].view(np.uint32)), len(x)      # untouched: the bits of f32(x g0)
        assert np.all(z[np.isnan(s)] == 0.0)
    assert untouched > 0
    print(f"{rate} Hz, true_peak={true_peak}: worst error / bound {worst:.3f} over N = {[len(s[0]) for s in _signals(rate)]}, "
          f"{untouched} untouched samples")
    return got


@pytest.mark.parametrize("rate", RATES)
def test_the_meter_is_the_peak_of_the_resampler_it_fuses_and_the_direct_sum(rate):
    sig = _signals(rate)
    x, starts, spans, u = _oversampled(rate)
    got = O.true_peak_seq(x, [(starts[i], len(sig[i][0])) for i in range(len(sig))]).cpu()
    want = O.peak_seq(u, spans).cpu()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    K = R.params(1, 4)[3]
    assert R.params(1, 4) == (4, 1, 96, 49)
    for i, (xs, _) in enumerate(sig):
        ref_u, mag = LM.oversample(xs)
        ref = LM.peak_of(ref_u)
        bound = (K + 1) * U * LM.peak_of(mag)                      # the forward bound of the chain, at whichever output holds the maximum
        print(f"{rate} Hz, N {len(xs)}: true peak {float(got[i]):.7f}, f64 {ref:.7f}, sample peak {LM.peak_of(xs):.7f}")
        assert abs(float(got[i]) - ref) <= bound, len(xs)
    assert float(got[0]) == 0.0                                     # the empty sequence


def test_the_quarter_rate_sine_reads_3_db_over_its_sample_peak():
    n = 2000
    x = np.sin(2 * np.pi * 0.25 * np.arange(n) + np.pi / 4).astype(F32)
    ramp = np.minimum(1.0, np.minimum(np.arange(n), np.arange(n)[::-1]) / 500.0)
    fade = (0.5 - 0.5 * np.cos(np.pi * ramp)).astype(F32)          # raised-cosine ends: no truncation to ring
    tp = O.measure_true_peak(x * fade, DEV)
    sp = 20 * np.log10(float(np.abs(x * fade).max()))
    ref_u, mag = LM.oversample(x * fade)
    ref = LM.peak_of(ref_u)
    print(f"fs/4 sine at 45 degrees: sample peak {sp:.4f} dBFS, true peak {tp:.5f} dBTP, f64 {20 * np.log10(ref):.5f} dBTP")
    assert abs(10.0 ** (tp / 20.0) - ref) <= (R.params(1, 4)[3] + 1) * U * LM.peak_of(mag) + 1e-12       # the meter's bound; 1e-12: the dB round trip
    assert abs(sp + 3.0103) <= 1e-3 and tp - sp > 3.0              # the 3 dB the sample-peak meter is blind to
    assert O.measure_true_peak(np.zeros(10, F32), DEV) == float("-inf") and O.measure_true_peak(np.zeros(0, F32), DEV) == float("-inf")
    assert O.measure_true_peak(_dev(x * fade)) == tp


@pytest.mark.parametrize("rate", RATES)
def test_sample_mode_against_f64_holds_the_ceiling_exactly(rate):
    mags = [LM.magnitude_sample(x, g0) for x, g0 in _signals(rate)]
    _check_against_f64(rate, False, mags)


@pytest.mark.parametrize("rate", RATES)
def test_sample_mode_statistics_and_bits_are_the_f32_arithmetic_of_the_definitions(rate):
    got, stats = _forward(rate, False)
    for i, (x, g0) in enumerate(_signals(rate)):
        z32, G32 = LM.limiter_f32(LM.scaled(x, g0), LM.magnitude_sample(x, g0), rate, LIMIT)
        assert np.array_equal(got[i].view(np.uint32), z32.view(np.uint32)), len(x)
        want = np.array([G32.min() if len(x) else 1.0, np.abs(got[i]).max() if len(x) else 0.0], F32)
        assert np.array_equal(stats[i].view(np.uint32), want.view(np.uint32)), (len(x), stats[i], want)
        assert len(x) == 0 or (stats[i][0] < 1.0 and stats[i][1] <= LM.ceiling(LIMIT))


@pytest.mark.parametrize("rate", RATES)
def test_true_peak_mode_against_f64_over_the_device_magnitudes(rate):
    sig = _signals(rate)
    _, _, spans, u = _oversampled(rate)
    u = u.cpu().numpy()
    mags = [LM.magnitude_true_peak(u[a: a + m], len(x), g0) for (a, m), (x, g0) in zip(spans, sig)]
    got = _check_against_f64(rate, True, mags)
    _, stats = _forward(rate, True)
    # the delivered true peak, against the reference's: the meter's own bound plus the limiter's error through the prototype's largest phase
    h = R.prototype_f32(1, 4)
    phase = max(float(np.abs(h[p::4]).sum()) for p in range(4))
    K, La = R.params(1, 4)[3], LM.lookahead(rate)
    order = list(range(len(sig)))
    z_dev, starts = _pack([got[i] for i in order], order)
    tp = O.true_peak_seq(z_dev, [(starts[i], len(got[i])) for i in order]).cpu().numpy()
    for i, (x, g0) in enumerate(sig):
        s = LM.scaled(x, g0)
        z_ref, _ = LM.limiter(s, mags[i], rate, LIMIT)
        ref_u, mag = LM.oversample(z_ref)
        bound = (K + 1) * U * LM.peak_of(mag) + phase * (La + 5) * U * LM.peak_of(s)
        ref = LM.peak_of(ref_u)
        if ref > 0:
            print(f"{rate} Hz, N {len(x)}: delivered true peak {20 * np.log10(max(float(tp[i]), 1e-30)):.5f} dBTP, reference "
                  f"{20 * np.log10(ref):.5f} dBTP, limit {LIMIT} dBTP")
        assert abs(float(tp[i]) - ref) <= bound, len(x)
        assert float(stats[i][1]) == (float(np.abs(got[i]).max()) if len(x) else 0.0)


@pytest.mark.parametrize("true_peak", [False, True])
@pytest.mark.parametrize("rate", RATES)
def test_every_sequence_keeps_its_bits_in_any_launch(rate, true_peak):
    first, first_stats = _forward(rate, true_peak)
    order = list(range(len(first)))
    for again in (order, order[::-1]):                              # a second run, and the other batch order
        got, stats = _limit_packed(rate, tuple(again), true_peak)
        for i in order:
            assert np.array_equal(got[i].view(np.uint32), first[i].view(np.uint32)), (len(first[i]), again[0])
            assert np.array_equal(stats[i].view(np.uint32), first_stats[i].view(np.uint32))
    for i in order:                                                 # and each sequence alone
        got, stats = _limit_packed(rate, (i,), true_peak)
        assert np.array_equal(got[i].view(np.uint32), first[i].view(np.uint32)), len(first[i])
        assert np.array_equal(stats[i].view(np.uint32), first_stats[i].view(np.uint32))


@pytest.mark.parametrize("true_peak", [False, True])
@pytest.mark.parametrize("rate", RATES)
def test_stream_pieces_are_bitwise_the_one_shot_output(rate, true_peak):
    """every split pattern as one stream each, advanced together through `deliver`: resampled, limited and encoded as f32 piece by piece"""
    N = 400
    rng = np.random.default_rng(rate + 7)
    fmt = O.AudioFormat(rate, "pcm_f32le", gain_db=14.0, limit_dbfs=LIMIT, true_peak=true_peak)
    xs = [rng.uniform(-0.4, 0.4, N).astype(F32) for _ in R.SPLITS]          # x 5: over the ceiling at every rate, 8 kHz's low-passed noise too
    plans = [R.splits(kind, N, rng) for kind in R.SPLITS]
    report = []
    whole = O.convert([_dev(x) for x in xs], None, [[i] for i in range(len(xs))], fmt, limiter_report=report)
    plain = O.convert([_dev(x) for x in xs], None, [[i] for i in range(len(xs))], O.AudioFormat(rate, "pcm_f32le"))
    streams = [O.OutputStream(fmt, 0) for _ in xs]
    got, pos, mixed = [[] for _ in xs], [0] * len(xs), False
    for k in range(max(map(len, plans))):
        idx = [i for i in range(len(xs)) if k < len(plans[i])]
        lasts = [k == len(plans[i]) - 1 for i in idx]
        mixed |= len(set(lasts)) == 2
        pieces = O.deliver([streams[i] for i in idx], [_dev(xs[i][pos[i]: pos[i] + plans[i][k]]) for i in idx], lasts)
        for i, p in zip(idx, pieces):
            got[i].append(p)
            pos[i] += plans[i][k]
    assert mixed
    c = LM.ceiling(LIMIT)
    for i, kind in enumerate(R.SPLITS):
        cat = np.concatenate(got[i])
        assert streams[i].finished and streams[i].lim_in == streams[i].lim_out == len(cat) == len(plain[i]), kind
        assert cat.dtype == np.float32 and np.array_equal(cat.view(np.uint32), whole[i].view(np.uint32)), kind
        assert np.abs(plain[i]).max() * fmt.gain > c and (true_peak or np.abs(cat).max() <= c)
        print(f"{rate} Hz, true_peak={true_peak}, {kind}: {report[i]}")
        assert report[i]["max_reduction_db"] > 0.5 and (true_peak or report[i]["peak_dbfs_after"] <= 20 * np.log10(float(c)))
    # the delay is the reach and no more: a first piece of R + 1 samples at the delivery rate lets exactly one sample out
    if rate == SRC:
        Rr = O.limiter_reach(rate, true_peak)
        s = O.OutputStream(fmt, 0)
        assert len(O.deliver([s], [_dev(xs[0][: Rr])], [False])[0]) == 0
        assert len(O.deliver([s], [_dev(xs[0][Rr: Rr + 1])], [False])[0]) == 1 and s.lim_out == 1 and int(s.lim_carry.numel()) == Rr + 1


def test_bad_arguments_are_refused_before_any_launch():
    L = _lib.lib()
    x = torch.zeros(64, device=DEV)
    tab = _dev([(0, 64, 0, 0, 0, 64, 1, 0)], np.int64)
    w, p, st = O.limiter_window(8000, DEV), _lib.ptr(x), _lib.stream_ptr(DEV)
    ok = dict(n_seq=1, max_n=64, la=40, c=0.5)
    for change in (dict(n_seq=0), dict(n_seq=65536), dict(max_n=-1), dict(la=0), dict(la=1025), dict(c=0.0), dict(c=1.5), dict(c=float("nan")),
                   dict(c=-0.5)):
        a = dict(ok, **change)
        rc = L.itts_pcm_limiter_seq_forward(p, p, _lib.ptr(w), None, _lib.ptr(tab), a["n_seq"], a["max_n"], a["la"], p, a["c"], None, st)
        assert rc == _lib.ERR_ARG and b"pcm_limiter_seq" in L.itts_last_error(), change
    for nulls in range(5):                                          # x, z, window, seq, gain
        args = [p, p, _lib.ptr(w), _lib.ptr(tab), p]
        args[nulls] = None
        assert L.itts_pcm_limiter_seq_forward(args[0], args[1], args[2], None, args[3], 1, 64, 40, args[4], 0.5, None, st) == _lib.ERR_ARG
    t4 = _lib.ptr(O.resample_table(1, 4, DEV))
    two = _dev([(0, 64)], np.int64)
    for args in ((None, p, t4, _lib.ptr(two), 1, 64), (p, None, t4, _lib.ptr(two), 1, 64), (p, p, None, _lib.ptr(two), 1, 64),
                 (p, p, t4, None, 1, 64), (p, p, t4, _lib.ptr(two), 0, 64), (p, p, t4, _lib.ptr(two), 1, -1)):
        assert L.itts_pcm_truepeak_seq_forward(*args, st) == _lib.ERR_ARG and b"pcm_truepeak_seq" in L.itts_last_error()
    torch.cuda.synchronize()
    assert not x.any()                                              # nothing ran
    assert O.limiter_seq(x, [(0, 64, 0, 0, 0, 0, 0)], 8000, 1.0, -1.0, False, 0).numel() == 1      # nothing to do: no launch
