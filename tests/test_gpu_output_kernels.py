"""The delivery-format kernels (csrc/pcm_kernels.hip; include/indextts_hip.h, "delivery formats") against the f64 restatements of
tests/pcm_ref.py: the resampler at its edges and as a stream, the encoders on every 16-bit value, the peak and the stream pieces."""
import numpy as np
import pytest
import torch

from indextts_amd import _lib, output as O
from tests import pcm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SRC = 22050
U = 2.0 ** -24
GUARD = 12345.0


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dtype))).to(DEV)


def _lengths(rate):
    """N in {1, 2, K - 1, K, K + 1} and the lengths whose N_out runs from just under the tile size to just over it"""
    L, M, H, K = R.params(SRC, rate)
    tile = O.RESAMPLE_TILE
    ns = [1, 2, K - 1, K, K + 1]
    at = tile * M // L                                              # N_out is near the tile size around here
    below = max(n for n in range(1, at + 2) if R.out_len(n, L, M) < tile)
    above = min(n for n in range(at, at + M + 2) if R.out_len(n, L, M) > tile)
    ns += list(range(below, above + 1))                             # the nearest lengths on both sides of the tile size (an integer
    outs = [R.out_len(n, L, M) for n in ns]                         # up-sampling ratio skips some output lengths) and all between
    assert tile - 3 <= min(outs[5:]) < tile < max(outs) <= tile + 3 and len(ns) <= 5 + M // L + 3
    return ns


def _resample_packed(xs, rate, order):
    """one launch over the sequences in `order`, NaN canaries between the packed inputs, guard values around every output"""
    L, M, H, K = R.params(SRC, rate)
    gap = 5
    x_parts, seqs, x_pos, y_pos = [np.full(gap, np.nan, np.float32)], [], gap, gap
    for i in order:
        n, n_out = len(xs[i]), R.out_len(len(xs[i]), L, M)
        x_parts += [xs[i], np.full(gap, np.nan, np.float32)]
        seqs.append((x_pos, n, 0, y_pos, 0, n_out, 1, 0))
        x_pos, y_pos = x_pos + n + gap, y_pos + n_out + gap
    x = _dev(np.concatenate(x_parts))
    y = torch.full((y_pos,), GUARD, dtype=torch.float32, device=DEV)
    table = O.resample_table(SRC, rate, DEV)
    tab = _dev(seqs, np.int64)
    _lib.check(_lib.lib().itts_pcm_resample_seq_forward(_lib.ptr(x), _lib.ptr(y), _lib.ptr(table), _lib.ptr(tab), len(seqs),
                                                        max(s[5] for s in seqs), L, M, H, K, _lib.stream_ptr(DEV)), "pcm_resample_seq")
    y = y.cpu().numpy()
    outs, guards = {}, np.ones(y_pos, dtype=bool)
    for i, s in zip(order, seqs):
        outs[i] = y[s[3]: s[3] + s[5]].copy()
        guards[s[3]: s[3] + s[5]] = False
    assert np.all(y[guards] == GUARD), "a block wrote outside its sequence's output"
    return outs


@pytest.mark.parametrize("rate", R.RATES)
def test_resample_at_the_edges_against_f64(rate):
    L, M, H, K = R.params(SRC, rate)
    assert O.resample_params(SRC, rate) == (L, M, H, K)
    rng = np.random.default_rng(rate)
    xs = [rng.uniform(-1, 1, n).astype(np.float32) for n in _lengths(rate)]
    order = list(range(len(xs)))
    got = _resample_packed(xs, rate, order)
    h = R.prototype_f32(SRC, rate)
    worst = 0.0
    for i, x in enumerate(xs):
        y, mag = R.resample(x, SRC, rate, h)
        assert got[i].shape == y.shape == (R.out_len(len(x), L, M),)
        assert np.all(np.isfinite(got[i])), "a neighbour's canary leaked in"
        err, bound = np.abs(got[i].astype(np.float64) - y), (K + 2) * U * mag        # the forward bound of a K-term fma chain
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (len(x), float(err.max()))
    print(f"{SRC} -> {rate}: worst error / bound {worst:.3f} over N = {[len(x) for x in xs]}")
    back = _resample_packed(xs, rate, order[::-1])                  # the other batch order: every sequence keeps its bits
    for i in order:
        assert np.array_equal(got[i].view(np.uint32), back[i].view(np.uint32)), len(xs[i])
    alone = _resample_packed(xs, rate, [len(xs) - 1])
    assert np.array_equal(alone[len(xs) - 1].view(np.uint32), got[len(xs) - 1].view(np.uint32))


def test_resample_refuses_bad_sizes_and_unready_outputs():
    L, M, H, K = O.resample_params(SRC, 8000)
    x = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError, match="has not arrived"):
        O.resample_seq(x, [(0, 64, 0, 0, 0, 5, 0)], SRC, 8000, 5)   # non-final: 64 samples complete no output's support
    with pytest.raises(ValueError, match="outside its buffer"):
        O.resample_seq(x, [(0, 65, 0, 0, 0, 1, 1)], SRC, 8000, 1)
    with pytest.raises(ValueError, match="starts after"):
        O.resample_seq(x, [(0, 64, 100000, 0, 0, 1, 1)], SRC, 8000, 1)
    table = O.resample_table(SRC, 8000, DEV)
    tab = _dev([(0, 64, 0, 0, 0, 1, 1, 0)], np.int64)
    rc = _lib.lib().itts_pcm_resample_seq_forward(_lib.ptr(x), _lib.ptr(x), _lib.ptr(table), _lib.ptr(tab), 1, 1, L, M, H, K + 1, _lib.stream_ptr(DEV))
    assert rc == _lib.ERR_ARG and b"pcm_resample_seq" in _lib.lib().itts_last_error()
    assert O.resample_seq(x, [(0, 64, 0, 0, 0, 0, 0)], SRC, 8000, 0).numel() == 1      # nothing to do: no launch


@pytest.mark.parametrize("rate", R.RATES)
def test_stream_pieces_are_bitwise_the_one_shot_output(rate):
    """every split pattern of the host test as one stream each, advanced together: a launch mixes final and non-final sequences"""
    L, M, H, K = R.params(SRC, rate)
    N = 2 * K + 97
    rng = np.random.default_rng(rate + 1)
    fmt = O.AudioFormat(rate, "pcm_f32le")
    xs = [rng.uniform(-0.4, 0.4, N).astype(np.float32) for _ in R.SPLITS]      # (no overshoot past the f32 encoding's clamp at 1)
    plans = [R.splits(kind, N, rng) for kind in R.SPLITS]
    whole = O.convert([_dev(x) for x in xs], None, [[i] for i in range(len(xs))], fmt)
    streams = [O.OutputStream(fmt, 0) for _ in xs]
    got = [[] for _ in xs]
    pos = [0] * len(xs)
    mixed = False
    for k in range(max(map(len, plans))):
        idx = [i for i in range(len(xs)) if k < len(plans[i])]
        lasts = [k == len(plans[i]) - 1 for i in idx]
        mixed |= len(set(lasts)) == 2
        pieces = O.deliver([streams[i] for i in idx], [_dev(xs[i][pos[i]: pos[i] + plans[i][k]]) for i in idx], lasts)
        for i, p in zip(idx, pieces):
            got[i].append(p)
            pos[i] += plans[i][k]
    assert mixed
    for i, kind in enumerate(R.SPLITS):
        cat = np.concatenate(got[i])
        assert streams[i].finished and streams[i].n_in == N and streams[i].n_out == len(cat) == R.out_len(N, L, M), kind
        assert cat.dtype == np.float32 and np.array_equal(cat.view(np.uint32), whole[i].view(np.uint32)), kind
    y, mag = R.resample(xs[0], SRC, rate)                           # and the one-shot output is the definition's
    assert np.all(np.abs(whole[0].astype(np.float64) - y) <= (K + 2) * U * mag)


# ---- encode ---------------------------------------------------------------------------------------------------------------------------------
def _encode_inputs():
    q = np.arange(-32768, 32768, dtype=np.float64)
    ties = np.arange(-40, 40, dtype=np.float64) + 0.5
    x = np.concatenate([q / 32767.0, ties / 32767.0, -ties / 32767.0, (32766.5 / 32767.0, -32766.5 / 32767.0),
                        (1.5, -1.5, np.nan, np.inf, -np.inf, 0.0, -0.0)])
    return x.astype(np.float32)


@pytest.mark.parametrize("gain_db", [0.0, -6.0, 3.5])
@pytest.mark.parametrize("encoding", list(O.ENCODINGS))
def test_encode_every_16_bit_value_bitwise(encoding, gain_db):
    x = _encode_inputs()
    fmt = O.AudioFormat(SRC, encoding, gain_db=gain_db)
    n = len(x)
    xd = _dev(np.concatenate([x, x[::-1]]))                         # two sequences, the second reversed
    out = O.encode_seq(xd, [(0, n, n), (n, n, 0)], encoding, fmt.gain).cpu().numpy()
    assert out.dtype == fmt.dtype
    want = R.encode(x, encoding, fmt.gain)
    for got, ref in ((out[n:], want), (out[:n], want[::-1])):
        if encoding == "pcm_f32le":
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
        else:
            assert np.array_equal(got, ref)
    if gain_db == 0.0 and encoding == "pcm_s16le":                  # q / 32767 comes back as q
        assert np.array_equal(out[n: n + 65536][1:], np.arange(-32767, 32768, dtype=np.int16))


def test_peak_is_bitwise_and_ignores_nan():
    rng = np.random.default_rng(5)
    lens = [1, 63, 64, 65, 2048, 2049, 70001, 0]
    xs = [rng.standard_normal(n).astype(np.float32) * 10.0 ** rng.uniform(-3, 1) for n in lens]
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    x = _dev(np.concatenate(xs))
    peak = O.peak_seq(x, list(zip(starts, lens))).cpu()
    want = torch.stack([torch.from_numpy(v).abs().amax() if len(v) else torch.tensor(0.0) for v in xs])
    assert torch.equal(peak.view(torch.int32), want.view(torch.int32))
    with_nan = np.concatenate(xs).copy()
    with_nan[[0, 5, 100, 3000]] = np.nan
    lens2 = [int(sum(lens))]
    got = float(O.peak_seq(_dev(with_nan), [(0, lens2[0])]).cpu()[0])
    assert got == float(np.nanmax(np.abs(with_nan)))
    assert float(O.peak_seq(_dev([np.nan, np.nan]), [(0, 2)]).cpu()[0]) == 0.0


def test_peak_dbfs_gain_and_the_silent_sequence():
    rng = np.random.default_rng(6)
    x = rng.uniform(-0.3, 0.3, 4000).astype(np.float32)
    fmt = O.AudioFormat(SRC, "pcm_f32le", peak_dbfs=-1.0)
    xd = _dev(np.concatenate([x, x]))
    peak = _dev([0.0, np.abs(x).max()])                             # a peak of 0 -> a gain of 1: the samples come back as they are
    out = O.encode_seq(xd, [(0, 4000, 0), (4000, 4000, 4000)], "pcm_f32le", fmt.gain, peak).cpu().numpy()
    assert np.array_equal(out[:4000].view(np.uint32), x.view(np.uint32))
    g = np.float32(fmt.gain) / np.float32(np.abs(x).max())          # the f32 division the kernel does
    assert np.array_equal(out[4000:].view(np.uint32), R.encode_f32(x, g).view(np.uint32))
    rows = _dev(np.stack([np.zeros(4000, np.float32), x]))
    silent, loud = O.convert(rows, [4000, 4000], [[0], [1]], fmt)
    assert not silent.any() and np.array_equal(loud.view(np.uint32), out[4000:].view(np.uint32))
    assert abs(float(np.abs(loud).max()) - 10.0 ** (-1.0 / 20)) <= 2e-7


# ---- stream pieces --------------------------------------------------------------------------------------------------------------------------
def test_stream_pieces_against_crossfade_and_fade_out_in_f64():
    """the chunk sequences of five rows through `deliver` at 22050 / pcm_f32le (no resampling, no scaling: the piece kernel's own output):
    a long row, one whose last piece is at most 512 samples, one with a chunk shorter than the overlap, two that end by a flush"""
    ovlp = 768
    rng = np.random.default_rng(8)
    rows = [([4000, 3000, 2500], [False, False, True], False),
            ([2000, 500], [False, True], False),                     # (overlap 200) the last piece: 500 samples, no fade
            ([3000, 500, 2000], [False, False, True], False),        # 500 < ovlp
            ([3000, 2200], [False, False], True),                    # ends without a closing chunk: the 768 held-back samples are flushed, faded
            ([900], [False], True)]                                  # a flush of at most 512 samples: no fade
    ovlps = [ovlp, 200, ovlp, ovlp, 400]
    fmt = O.AudioFormat(SRC, "pcm_f32le")
    streams = [O.OutputStream(fmt, o) for o in ovlps]
    tails = [None] * len(rows)
    steps = max(len(r[0]) + int(r[2]) for r in rows)
    checked = dict(blend=0, fade=0, short_last=0, short_chunk=0, flush=0)
    for k in range(steps):
        idx = [i for i, r in enumerate(rows) if k < len(r[0]) + int(r[2])]
        audio = [rng.uniform(-0.9, 0.9, rows[i][0][k]).astype(np.float32) if k < len(rows[i][0]) else None for i in idx]
        lasts = [bool(a is not None and rows[i][1][k]) for i, a in zip(idx, audio)]
        got = O.deliver([streams[i] for i in idx], [None if a is None else _dev(a) for a in audio], lasts)
        for i, a, last, g in zip(idx, audio, lasts, got):
            want, keep, mag = R.piece(tails[i], a, ovlps[i], last)
            assert g.dtype == np.float32 and g.shape == want.shape, (i, k)
            assert np.all(np.abs(g.astype(np.float64) - want) <= 3 * U * mag), (i, k)
            if a is None or last:
                assert streams[i].tail is None and streams[i].finished
            else:
                assert np.array_equal(streams[i].tail.cpu().numpy(), keep.astype(np.float32)), (i, k)
            checked["blend"] += tails[i] is not None and a is not None
            checked["fade"] += (a is None or last) and len(want) > 512
            checked["short_last"] += bool(last) and len(want) <= 512
            checked["short_chunk"] += a is not None and len(a) < ovlps[i]
            checked["flush"] += a is None
            tails[i] = keep
    assert all(v > 0 for v in checked.values()), checked
    assert O.deliver([O.OutputStream(fmt, ovlp)], [None], [False]) == [None]        # a stream that never got a chunk has nothing to flush


def test_convert_assembles_resamples_and_encodes_whole_requests():
    rng = np.random.default_rng(9)
    lens = [700, 1300, 1, 999]
    rows = np.zeros((4, 1400), np.float32)
    for i, n in enumerate(lens):
        rows[i, :n] = rng.uniform(-0.8, 0.8, n)
        rows[i, n:] = np.nan                                        # past a row's length: never read
    groups = [[1, 0, 3], [2], [3, 1]]
    sil = int(SRC * 40 / 1000.0)
    whole = [np.concatenate(sum([[rows[i, : lens[i]], np.zeros(sil, np.float32)] for i in g], [])[:-1]) for g in groups]
    f32 = O.convert(_dev(rows), lens, groups, "22050/pcm_f32le", interval_silence=40)
    for a, b in zip(f32, whole):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for spec in ("8000/mulaw", "48000/pcm_s16le", "16000/alaw"):
        fmt = O.AudioFormat.parse(spec)
        L, M, H, K = R.params(SRC, fmt.sample_rate)
        got = O.convert(_dev(rows), lens, groups, fmt, interval_silence=40)
        alone = O.convert([_dev(w) for w in whole], None, [[0], [1], [2]], fmt)
        y32 = O.convert([_dev(w) for w in whole], None, [[0], [1], [2]], O.AudioFormat(fmt.sample_rate, "pcm_f32le"))
        for g, a, y, w in zip(got, alone, y32, whole):
            assert g.dtype == fmt.dtype and len(g) == R.out_len(len(w), L, M) and np.array_equal(g, a)
            assert np.array_equal(g, R.encode(y, fmt.encoding))     # the encoding of the resampled floats
    assert O.convert(_dev(rows), lens, [], "8000/mulaw") == []
