"""The loudness kernels (csrc/loudness_kernels.hip; include/indextts_hip.h, "loudness normalisation") against the f64 restatement of
tests/loudness_ref.py: packed ragged batches at three rates with the lengths around the shortest measurable one, both gates biting, a NaN
sample, NaN canaries between the sequences; the same bits in the other batch order, alone and on a second run; a sequence long enough for
every kernel's second tile; the peak found on the way; the gain entry bit for bit against its formula."""
import math

import numpy as np
import pytest
import torch

from indextts_amd import _lib, output as O
from tests import loudness_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATES = (8000, 22050, 48000)
TOL_LU = 1e-6            # 2.3e-7 relative in the mean square: nine orders above f64 roundoff, five under a meter's resolution
GAP = 5


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def _noise(rng, n, amp):
    return (amp * rng.uniform(-1.0, 1.0, n)).astype(np.float32)


def _sequences(rate):
    """lengths 0, 4 hop - 1, 4 hop, 4 hop + 1, 7 hop + 3 (one NaN sample inside) and about 2.5 s in three sections: near silence (under the absolute
    gate), 25 dB under the last (under the relative gate), and the loud one"""
    h = LR.hop(rate)
    rng = np.random.default_rng(rate)
    xs = [_noise(rng, n, 0.25) for n in (0, 4 * h - 1, 4 * h, 4 * h + 1)]
    x = np.concatenate([_noise(rng, 3 * h + 1, 0.02), _noise(rng, 4 * h + 2, 0.4)])
    x[3 * h + 7] = np.nan
    xs.append(x)
    loud = 0.3
    xs.append(np.concatenate([_noise(rng, 8 * h, 1e-5), _noise(rng, 7 * h, loud * 10.0 ** (-25.0 / 20.0)), _noise(rng, 10 * h + h // 3, loud)]))
    assert [len(x) for x in xs[:5]] == [0, 4 * h - 1, 4 * h, 4 * h + 1, 7 * h + 3] and abs(len(xs[5]) / rate - 2.5) < 0.05
    return xs


_refs = {}


def _reference(rate):
    """the sequences of a rate and their reference measurement, computed once"""
    if rate not in _refs:
        xs = _sequences(rate)
        _refs[rate] = (xs, [LR.measure(x, rate) for x in xs])
    return _refs[rate]


def _measure_packed(xs, rate, order, want_peak=False):
    """one call over the sequences in `order`, NaN canaries between them -> {index: f64 LUFS}, {index: f32 peak}"""
    parts, seqs, pos = [np.full(GAP, np.nan, np.float32)], [], GAP
    for i in order:
        parts += [xs[i], np.full(GAP, np.nan, np.float32)]
        seqs.append((pos, len(xs[i])))
        pos += len(xs[i]) + GAP
    lufs, peak = O._measure_seq(_dev(np.concatenate(parts)), seqs, rate, want_peak, "test")
    lufs = lufs.cpu().numpy()
    assert lufs.dtype == np.float64 and lufs.shape == (len(order),)
    peaks = dict(zip(order, peak.cpu().numpy())) if want_peak else None
    return dict(zip(order, lufs)), peaks


@pytest.mark.parametrize("rate", RATES)
def test_packed_batch_against_the_f64_reference(rate):
    xs, refs = _reference(rate)
    long_ref = refs[5]
    print(f"{rate} Hz, the 2.5 s sequence: {long_ref['kept_abs']} / {long_ref['kept']} of {long_ref['n_blocks']} blocks through the absolute / "
          f"both gates, nearest block {long_ref['margin']:.2f} LU from a gate")
    assert long_ref["kept"] < long_ref["kept_abs"] < long_ref["n_blocks"], "both gates must bite"
    assert all(m["margin"] >= 0.5 for m in refs), "a block of the reference lies on a gate: no test of the kernel"
    assert [m["n_blocks"] for m in refs[:5]] == [0, 0, 1, 1, 4] and all(math.isfinite(m["lufs"]) for m in refs[2:])
    order = list(range(len(xs)))
    got, _ = _measure_packed(xs, rate, order)
    worst = 0.0
    for i, m in enumerate(refs):
        if m["lufs"] == -math.inf:
            assert got[i] == -math.inf, (i, got[i])
            continue
        assert math.isfinite(got[i]), (i, got[i])                    # neither the NaN sample nor a neighbour's canary leaked in
        worst = max(worst, abs(got[i] - m["lufs"]))
    print(f"{rate} Hz: max |L_device - L_ref| = {worst:.3e} LU over N = {[len(x) for x in xs]}")
    assert worst <= TOL_LU
    # the same bits on a second run, in the other batch order, and alone
    again, _ = _measure_packed(xs, rate, order)
    back, _ = _measure_packed(xs, rate, order[::-1])
    for i in order:
        alone, _ = _measure_packed(xs, rate, [i])
        bits = np.float64(got[i]).view(np.uint64)
        assert bits == np.float64(again[i]).view(np.uint64) == np.float64(back[i]).view(np.uint64) == np.float64(alone[i]).view(np.uint64), i
    # the public wrapper is the same call
    pub = O.loudness_seq(_dev(np.concatenate([xs[5], xs[2]])), [(0, len(xs[5])), (len(xs[5]), len(xs[2]))], rate).cpu().numpy()
    assert pub[0].view(np.uint64) == np.float64(got[5]).view(np.uint64) and pub[1].view(np.uint64) == np.float64(got[2]).view(np.uint64)
    assert O.measure_loudness(_dev(xs[5]), rate) == got[5] and O.measure_loudness(xs[5], rate, DEV) == got[5]
    assert O.measure_loudness(np.zeros(0, np.float32), rate, DEV) == -math.inf


def test_a_sequence_past_every_kernels_first_tile():
    """103 s at 8 kHz: 1030 sub-blocks -- seventeen 64-lane blocks of the chunk kernels, seventeen rounds of the chain, and more 400 ms blocks than the
    gate kernel has threads -- in a batch with a short neighbour"""
    rate = 8000
    h = LR.hop(rate)
    rng = np.random.default_rng(7)
    n_sub = 1030
    # a new level every second, from three that keep every block -- those that straddle a change too -- clear of the relative gate
    amp = np.repeat(10.0 ** (rng.choice([-10.0, -14.0, -40.0], n_sub // 10) / 20.0), 10 * h)
    long = (amp * rng.uniform(-1.0, 1.0, n_sub * h)).astype(np.float32)
    short = _noise(rng, 5 * h + 11, 0.2)
    m, m_short = LR.measure(long, rate), LR.measure(short, rate)
    print(f"{m['kept']} of {m['n_blocks']} blocks kept, nearest block {m['margin']:.3f} LU from a gate")
    assert m["n_blocks"] == n_sub - 3 > 1024 and m["kept"] < m["kept_abs"] == m["n_blocks"]
    assert m["margin"] >= 0.5 and m_short["margin"] >= 0.5, "a block of the reference lies on a gate: no test of the kernel"
    got, peaks = _measure_packed([long, short], rate, [0, 1], want_peak=True)
    print(f"max |L_device - L_ref| = {max(abs(got[0] - m['lufs']), abs(got[1] - m_short['lufs'])):.3e} LU")
    assert abs(got[0] - m["lufs"]) <= TOL_LU and abs(got[1] - m_short["lufs"]) <= TOL_LU
    back, _ = _measure_packed([long, short], rate, [1, 0])
    assert np.float64(got[0]).view(np.uint64) == np.float64(back[0]).view(np.uint64)
    assert peaks[0] == np.abs(long).max() and peaks[1] == np.abs(short).max()


@pytest.mark.parametrize("rate", RATES)
def test_the_peak_found_on_the_way_is_the_peak_entrys(rate):
    xs, _ = _reference(rate)
    order = list(range(len(xs)))
    _, peaks = _measure_packed(xs, rate, order, want_peak=True)
    flat = _dev(np.concatenate(xs))
    starts = np.concatenate([[0], np.cumsum([len(x) for x in xs])])
    ref = O.peak_seq(flat, [(int(starts[i]), len(xs[i])) for i in order]).cpu().numpy()
    for i in order:
        want = np.float32(0.0) if len(xs[i]) == 0 else np.nanmax(np.abs(xs[i]))
        assert peaks[i].view(np.uint32) == ref[i].view(np.uint32) == np.float32(want).view(np.uint32), i      # the tail past the last sub-block too


def test_gain_entry_bit_for_bit():
    lufs = np.array([-20.3, -35.123456789, -math.inf, -12.0, -3.3, -41.7], dtype=np.float64)
    peak = np.array([0.5, 0.25, 0.3, 0.0, 0.9, 0.001], dtype=np.float32)
    d_lufs, d_peak = _dev(lufs, np.float64), _dev(peak)
    target, ceiling = -16.0, -3.0
    # target only
    g = O.loudness_gain(d_lufs, target).cpu().numpy()
    want = np.array([LR.gain(L, target) for L in lufs], dtype=np.float32)
    assert np.array_equal(g.view(np.uint32), want.view(np.uint32)) and g[2] == 1.0
    # a peak table without a ceiling changes nothing
    g2, rep = O.loudness_gain(d_lufs, target, d_peak, None, report=True)
    assert np.array_equal(g2.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # with a ceiling: it binds for rows 0 and 1 (the target would lift their peaks above it); not for row 2 (L = -inf: g = 1, and 0.3 lies under
    # it), row 3 (peak 0), rows 4 and 5
    g3, rep3 = O.loudness_gain(d_lufs, target, d_peak, ceiling, report=True)
    g3 = g3.cpu().numpy()
    want3 = np.array([LR.gain(L, target, p, ceiling) for L, p in zip(lufs, peak)], dtype=np.float32)
    assert np.array_equal(g3.view(np.uint32), want3.view(np.uint32))
    ceil_lin = np.float32(10.0 ** (ceiling / 20.0))
    binds = [bool(w * p > ceil_lin) for w, p in zip(want, peak)]
    assert binds == [True, True, False, False, False, False]
    for i, b in enumerate(binds):
        assert (g3[i] == np.float32(ceil_lin / peak[i])) if b else (g3[i] == want[i]), i
    assert g3[2] == 1.0 and g3[3] == want[3]
    # the report: L, the gain in dB, the delivered peak in dBFS
    rep3 = rep3.cpu().numpy()
    assert np.array_equal(rep3[:, 0].view(np.uint64), lufs.view(np.uint64))
    assert np.max(np.abs(rep3[:, 1] - 20.0 * np.log10(g3.astype(np.float64)))) <= 1e-12
    with np.errstate(divide="ignore"):
        after = 20.0 * np.log10(np.minimum(g3 * peak, np.float32(1.0)).astype(np.float64))
    assert rep3[3, 2] == -math.inf and np.max(np.abs(np.delete(rep3[:, 2], 3) - np.delete(after, 3))) <= 1e-12
    assert abs(rep3[0, 2] - ceiling) <= 1e-6 and abs(rep3[1, 2] - ceiling) <= 1e-6


def test_entries_refuse_bad_sizes_before_any_launch():
    x = _dev(np.zeros(100, np.float32))
    lufs = torch.zeros(1, dtype=torch.float64, device=DEV)
    tab = _dev([[0, 100, 0, 0]], np.int64)
    work = torch.zeros(9, dtype=torch.float64, device=DEV)
    L = _lib.lib()
    st = _lib.stream_ptr(DEV)
    assert L.itts_pcm_loudness_seq_forward(_lib.ptr(x), _lib.ptr(lufs), None, _lib.ptr(tab), 1, 100, 8000, 4, _lib.ptr(work), 72, st) == _lib.ERR_ARG
    assert L.itts_pcm_loudness_seq_forward(_lib.ptr(x), _lib.ptr(lufs), None, _lib.ptr(tab), 1, 100, 8000, 0, _lib.ptr(work), 72, st) == 0
    torch.cuda.synchronize()
    assert lufs.cpu()[0] == -math.inf
