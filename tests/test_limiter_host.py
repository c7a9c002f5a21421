"""The look-ahead limiter and the true-peak ceiling without a GPU: the format's new fields and every refusal, the integer
rules of the streaming limiter against brute force, the smoothing window, and the f64 restatement of tests/limiter_ref.py checked against the
properties the definitions promise -- so the oracle the GPU tests compare with is known good."""
import math
import os

import numpy as np
import pytest

from indextts_amd import output as O
from tests import limiter_ref as LM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 22050, 48000)
F32 = np.float32


# ---- AudioFormat ----------------------------------------------------------------------------------------------------------------------------
def test_audio_format_carries_the_limiter_in_key_equality_and_hash():
    plain, lim = O.AudioFormat(48000, "pcm_f32le"), O.AudioFormat(48000, "pcm_f32le", limit_dbfs=-1)
    tp = O.AudioFormat(48000, "pcm_f32le", limit_dbfs=-1, true_peak=True)
    assert plain.limit_dbfs is None and plain.true_peak is False and plain.ceiling is None
    assert lim.limit_dbfs == -1.0 and isinstance(lim.limit_dbfs, float) and lim.true_peak is False and tp.true_peak is True
    assert lim.ceiling == F32(10.0 ** (-1.0 / 20)) and lim.ceiling.dtype == np.float32
    assert len({plain, lim, tp, O.AudioFormat(48000, "pcm_f32le", limit_dbfs=-2)}) == 4 and lim == O.AudioFormat(48000, "pcm_f32le", limit_dbfs=-1.0)
    assert hash(tp) == hash(O.AudioFormat(48000, "pcm_f32le", limit_dbfs=-1.0, true_peak=True))
    assert lim.key() == (48000, "pcm_f32le", 0.0, None, None, -1.0, False) and tp.key() == (48000, "pcm_f32le", 0.0, None, None, -1.0, True)
    assert O.AudioFormat(8000, "mulaw", peak_dbfs=-1.0, true_peak=True).key() == (8000, "mulaw", 0.0, -1.0, None, None, True)
    both = O.AudioFormat(48000, loudness_lufs=-16, limit_dbfs=-1, true_peak=True)            # the point of the feature: a target AND a ceiling
    assert both.key() == (48000, "pcm_s16le", 0.0, None, -16.0, -1.0, True)
    assert O.AudioFormat(8000, gain_db=6.0, limit_dbfs=-1).gain == F32(10.0 ** (6.0 / 20))   # a fixed gain in front of the limiter: a stream's form
    with pytest.raises(AttributeError):
        lim.limit_dbfs = -2.0
    for edge in (0.0, -0.0, -60.0):
        assert O.AudioFormat(limit_dbfs=edge).limit_dbfs == edge


def test_formats_without_the_new_fields_keep_their_key_and_repr():
    assert O.AudioFormat().key() == (22050, "pcm_s16le", 0.0, None, None)
    assert O.AudioFormat(8000, "mulaw", peak_dbfs=-1.0, loudness_lufs=-16).key() == (8000, "mulaw", 0.0, -1.0, -16.0)
    assert repr(O.AudioFormat()) == "AudioFormat(sample_rate=22050, encoding='pcm_s16le', gain_db=0.0, peak_dbfs=None)"
    assert repr(O.AudioFormat(48000, "pcm_f32le", loudness_lufs=-16)) == \
        "AudioFormat(sample_rate=48000, encoding='pcm_f32le', gain_db=0.0, peak_dbfs=None, loudness_lufs=-16.0)"
    assert repr(O.AudioFormat(48000, "pcm_f32le", limit_dbfs=-1)) == \
        "AudioFormat(sample_rate=48000, encoding='pcm_f32le', gain_db=0.0, peak_dbfs=None, limit_dbfs=-1.0)"
    assert repr(O.AudioFormat(48000, loudness_lufs=-16, limit_dbfs=-1, true_peak=True)) == \
        "AudioFormat(sample_rate=48000, encoding='pcm_s16le', gain_db=0.0, peak_dbfs=None, loudness_lufs=-16.0, limit_dbfs=-1.0, true_peak=True)"
    assert repr(O.AudioFormat(peak_dbfs=-1, true_peak=True)) == \
        "AudioFormat(sample_rate=22050, encoding='pcm_s16le', gain_db=0.0, peak_dbfs=-1.0, true_peak=True)"


def test_audio_format_dict_and_string_forms():
    want = O.AudioFormat(48000, "pcm_s16le", loudness_lufs=-16.0, limit_dbfs=-1.0, true_peak=True)
    assert O.AudioFormat.parse("48000/pcm_s16le/-16lufs/-1limit/tp") == want
    assert O.AudioFormat.parse("tp/-1 LIMIT/-16lufs/pcm_s16le/48000") == want                 # any order, any case
    assert O.AudioFormat.parse(dict(sample_rate=48000, loudness_lufs=-16, limit_dbfs=-1, true_peak=True)) == want
    assert O.AudioFormat.parse("8000/mulaw/-1.5limit") == O.AudioFormat(8000, "mulaw", limit_dbfs=-1.5)
    assert O.AudioFormat.parse("-3limit") == O.AudioFormat(limit_dbfs=-3.0)
    assert O.AudioFormat.parse("-0limit/tp") == O.AudioFormat(limit_dbfs=0.0, true_peak=True)
    assert O.AudioFormat.parse("48000/pcm_s16le").limit_dbfs is None and O.AudioFormat.parse("48000/pcm_s16le").true_peak is False


@pytest.mark.parametrize("bad, match", [
    (dict(limit_dbfs=0.5), "<= 0"), (dict(limit_dbfs=float("nan")), "finite"), (dict(limit_dbfs=float("-inf")), "finite"),
    (dict(limit_dbfs="hard"), "number"), (dict(limit_dbfs=-1, peak_dbfs=-1), "limit_dbfs or peak_dbfs, not both"),
    (dict(limit_dbfs=-1, peak_dbfs=-1, loudness_lufs=-16), "not both"), (dict(true_peak=True), "true_peak needs peak_dbfs or limit_dbfs"),
    (dict(true_peak=True, loudness_lufs=-16), "true_peak needs"), (dict(true_peak=1, limit_dbfs=-1), "true_peak must be a bool"),
    (dict(sample_rate=99, limit_dbfs=-1), "look-ahead"), (dict(sample_rate=204900, limit_dbfs=-1), "look-ahead|not supported"),
    (dict(limit_dbfs=-1, loudness_lufs=-16, gain_db=2.0), "not both"), (dict(limit=-1), "unknown keys"),
    ("48000/-1limit/-2limit", "rate/encoding"), ("48000/tp/tp/-1limit", "rate/encoding"), ("48000/tp", "true_peak needs"),
    ("48000/pcm_s16le/-16lufs/-1limit/tp/x", "rate/encoding"), ("1limit", "<= 0"), ("48000/pcm_s16le/-1", "rate/encoding")])
def test_audio_format_refuses_bad_limiters(bad, match):
    with pytest.raises(ValueError, match=match):
        O.AudioFormat.parse(bad)


def test_stream_format_accepts_the_limiter_and_still_refuses_the_other_two():
    for spec in (dict(sample_rate=8000, limit_dbfs=-1.0), dict(limit_dbfs=-1.0, true_peak=True, gain_db=12.0), "48000/pcm_f32le/-1limit/tp"):
        f = O.stream_format(spec, "here")
        assert f == O.AudioFormat.parse(spec) and f.limit_dbfs == -1.0
        s = O.OutputStream(f, 10)
        assert s.fmt == f and s.lim_carry is None and s.lim_in == s.lim_out == 0
    with pytest.raises(ValueError, match="here: audio_format with peak_dbfs needs the whole request"):
        O.stream_format(dict(peak_dbfs=-1.0, true_peak=True), "here")
    with pytest.raises(ValueError, match="here: audio_format with loudness_lufs needs the whole request"):
        O.stream_format("48000/-16lufs/-1limit", "here")
    assert O.stream_format(None, "here") is None


def test_streaming_entries_take_the_limiter_and_whole_request_entries_check_it_before_any_engine_work():
    from tests.test_token_scores_host import _tts
    t = _tts()
    sess = t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global", audio_format=dict(sample_rate=8000, limit_dbfs=-1.0))
    assert sess.backend.audio_format == O.AudioFormat(8000, limit_dbfs=-1.0)
    with pytest.raises(ValueError, match="not both"):
        t.infer_requests([dict(spk_audio_prompt="a.wav", text="hello", lang="en", audio_format=dict(limit_dbfs=-1, peak_dbfs=-1))], num_beams=1)
    with pytest.raises(ValueError, match="true_peak needs"):
        t.infer_batch("a.wav", ["hello"], "en", audio_format=dict(true_peak=True))
    with pytest.raises(ValueError, match="audio_format"):
        t.infer("a.wav", "hello", None, "en", audio_format="8000/-1limit")
    assert t.last_limiter is None and not t.gpt.calls


# ---- integers and the window ------------------------------------------------------------------------------------------------------------------
def test_lookahead_and_reach_at_the_named_rates():
    assert [O.limiter_lookahead(r) for r in RATES] == [40, 110, 240] == [LM.lookahead(r) for r in RATES]
    assert [O.limiter_reach(r, True) for r in RATES] == [64, 134, 264] and [O.limiter_reach(r, False) for r in RATES] == [40, 110, 240]
    assert O.limiter_lookahead(100) == 1 and O.limiter_lookahead(99) == 0 and O.limiter_lookahead(204899) == 1024 and O.limiter_lookahead(204900) == 1025
    assert O.resample_params(1, 4) == (4, 1, 96, 49) and O.ZERO_CROSSINGS == LM.Z == 24
    with pytest.raises(ValueError, match="look-ahead"):
        O.limiter_taps(99)


def test_header_and_binding_declare_the_limiter_entries():
    from indextts_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    L = _lib.lib()
    for name, nargs in (("itts_pcm_limiter_lookahead", 1), ("itts_pcm_truepeak_seq_forward", 7), ("itts_pcm_limiter_seq_forward", 12)):
        assert name + "(" in hdr and hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert f"#define ITTS_PCM_LIMITER_TILE {O.LIMITER_TILE}" in hdr and f"#define ITTS_PCM_LIMITER_MAX_LOOKAHEAD {O.LIMITER_MAX_LOOKAHEAD}" in hdr
    for rate in RATES + (1, 99, 100, 204899, 204900, 384000):
        assert L.itts_pcm_limiter_lookahead(rate) == O.limiter_lookahead(rate), rate
    assert L.itts_pcm_limiter_lookahead(0) == 0 and L.itts_pcm_limiter_lookahead(-5) == 0
    # refused through itts_set_error before any launch (no device is touched)
    assert L.itts_pcm_limiter_seq_forward(None, None, None, None, None, 1, 1, 40, None, 0.5, None, None) == _lib.ERR_ARG
    assert b"pcm_limiter_seq" in L.itts_last_error()
    assert L.itts_pcm_truepeak_seq_forward(None, None, None, None, 1, 1, None) == _lib.ERR_ARG and b"pcm_truepeak_seq" in L.itts_last_error()


@pytest.mark.parametrize("rate", RATES + (100, 204899))
def test_the_window_sums_to_one_and_is_the_restatement(rate):
    w = O.limiter_taps(rate)
    La = O.limiter_lookahead(rate)
    assert w.dtype == np.float32 and w.shape == (La + 1,) and np.all(w > 0) and np.array_equal(w, w[::-1])
    assert abs(float(np.sum(w.astype(np.float64))) - 1.0) <= 1e-7
    assert np.array_equal(w.view(np.uint32), LM.window(rate).view(np.uint32))


@pytest.mark.parametrize("R", [0, 1, 40, 64, 264])
def test_ready_and_first_needed_against_brute_force(R):
    for n in list(range(0, 3 * R + 5)) + [1000, 1001]:
        assert O.limiter_ready(n, True, R) == LM.ready(n, True, R) == n
        assert O.limiter_ready(n, False, R) == LM.ready(n, False, R), n
        assert O.limiter_first_needed(n, R) == LM.first_needed(n, R), n
    # a stream's bookkeeping: every output is produced once, and what is carried always covers the next output's reach
    n_in = n_out = 0
    for piece, final in ((1, False), (R, False), (R + 1, False), (3, False), (500, False), (0, True)):
        n_in += piece
        ready = O.limiter_ready(n_in, final, R)
        assert ready >= n_out
        n_out = ready
        assert O.limiter_first_needed(n_out, R) <= n_out <= n_in
    assert n_out == n_in


# ---- the restatement is known good ------------------------------------------------------------------------------------------------------------
def _bursts(rate, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, n).astype(F32)
    x[n // 3: n // 3 + 7] *= F32(3.0)
    x[0], x[-1] = F32(1.4), F32(-1.3)
    return x


@pytest.mark.parametrize("rate", RATES)
def test_the_reference_holds_the_ceiling_and_leaves_quiet_regions_alone(rate):
    La, c = LM.lookahead(rate), float(LM.ceiling(-1.0))
    x = _bursts(rate, 4 * La + 300, rate)
    for g0 in (1.0, 1.7):
        s, a = LM.scaled(x, g0), LM.magnitude_sample(x, g0)
        z, G = LM.limiter(s, a, rate, -1.0)
        before = np.abs(s.astype(np.float64) * G).max() / c - 1.0
        print(f"{rate} Hz, g0 {g0}: max |s G| / c - 1 = {before:.3e}, min G {G.min():.6f}")
        assert np.all(np.abs(z) <= c) and before <= 1e-7 and G.min() < 1.0 and np.all(G > 0.0) and np.all(G <= 1.0)
        hot = np.flatnonzero(a.astype(np.float64) > c)
        near = np.zeros(len(x), bool)
        for i in hot:
            near[max(0, i - La): i + La + 1] = True
        assert near.any() and (~near).any()
        assert np.all(G[~near] == 1.0) and np.array_equal(z[~near], s[~near].astype(np.float64))        # untouched: the bits of f32(x g0)
        assert np.all(G[hot] <= c / a[hot].astype(np.float64) * (1 + 1e-12))                            # at a hot sample the gain is low enough
        z32, G32 = LM.limiter_f32(s, a, rate, -1.0)                 # the f32 form: the same function to the GPU tests' tolerance, the ceiling exact
        assert np.all(np.abs(z32.astype(np.float64) - z) <= (La + 5) * 2.0 ** -24 * np.abs(s.astype(np.float64)))
        assert np.all(np.abs(z32) <= LM.ceiling(-1.0)) and np.array_equal(z32[~near].view(np.uint32), s[~near].view(np.uint32))
        assert np.all(G32[~near] == 1.0)


@pytest.mark.parametrize("rate", RATES)
def test_an_isolated_impulse_moves_the_gain_only_within_the_lookahead(rate):
    La = LM.lookahead(rate)
    n, at = 4 * La + 11, 2 * La + 3
    x = np.zeros(n, F32)
    x[at] = F32(4.0)                                               # 4x over full scale
    z, G = LM.limiter(LM.scaled(x, 1.0), LM.magnitude_sample(x, 1.0), rate, 0.0)
    inside = np.abs(np.arange(n) - at) <= La
    assert np.all(G[~inside] == 1.0) and np.all(G[inside] < 1.0) and abs(G[at] - 0.25) <= 1e-6 and abs(z[at] - 1.0) <= 1e-6
    assert G.argmin() == at and np.all(np.diff(G[: at + 1]) <= 0) and np.all(np.diff(G[at:]) >= 0)         # one smooth dip


def test_nan_asks_for_nothing_and_is_delivered_as_zero():
    x = np.array([0.1, np.nan, 0.2, 2.0, 0.1] + [0.05] * 100, F32)
    s, a = LM.scaled(x, 1.0), LM.magnitude_sample(x, 1.0)
    assert a[1] == 0.0
    z, _ = LM.limiter(s, a, 8000, -1.0)
    z32, _ = LM.limiter_f32(s, a, 8000, -1.0)
    assert z[1] == 0.0 and z32[1] == 0.0 and np.all(np.isfinite(z)) and np.all(np.isfinite(z32))


def test_the_f32_fma_is_exact_on_ties_and_plain_cases():
    a = np.array([1.0, 1.0 + 2.0 ** -23, 3.0, 1.0 + 2.0 ** -23], F32)
    b = np.array([1.0, 1.0 + 2.0 ** -23, 0.5, 1.0 - 2.0 ** -24], F32)
    c = np.array([2.0 ** -24, 0.0, 2.0 ** -30, 2.0 ** -60], F32)
    got = LM.fmaf(a, b, c)
    for i in range(len(a)):
        from fractions import Fraction
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], F32(-np.inf)), np.nextafter(got[i], F32(np.inf))
        d = abs(Fraction(float(got[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), i


def test_the_quarter_rate_sine_reads_0_dbtp_where_the_sample_peak_reads_minus_3():
    n = 400
    x = np.sin(2 * np.pi * 0.25 * np.arange(n) + np.pi / 4).astype(F32)
    assert abs(20 * math.log10(float(np.abs(x).max())) - (-3.0103)) <= 1e-3
    u, _ = LM.oversample(x)
    assert u.shape == (4 * n,)
    mid = 20 * math.log10(LM.peak_of(u[4 * 60: 4 * (n - 60)]))      # away from the truncated ends, which ring above it
    print(f"fs/4 sine at 45 degrees: {mid:.3e} dBTP away from the ends, {20 * math.log10(LM.peak_of(u)):.4f} dBTP with them")
    assert abs(mid) <= 1e-3
    a = LM.magnitude_true_peak(u.astype(F32), n, 1.0)
    assert a.dtype == np.float32 and abs(20 * math.log10(float(a[100: 300].max()))) <= 1e-3 and LM.true_peak(np.zeros(0, F32)) == 0.0
    assert LM.peak_of([np.nan, -0.5, 0.25]) == 0.5 and LM.peak_of([np.nan]) == 0.0


def test_wrappers_check_their_tables_before_any_launch():
    import torch
    x = torch.zeros(1000)
    for seqs in ([(0, 1001, 0, 0, 0, 1001, 1)], [(-1, 5, 0, 0, 0, 5, 1)], [(0, 10, 0, 995, 0, 10, 1)], [(0, 10, 0, 0, -1, 10, 1)]):
        with pytest.raises(ValueError, match="outside its buffer"):
            O.limiter_seq(x, seqs, 8000, 1.0, -1.0, False, 1000)
    with pytest.raises(ValueError, match="has not arrived"):
        O.limiter_seq(x, [(0, 100, 0, 0, 0, 61, 0)], 8000, 1.0, -1.0, False, 100)        # non-final, La 40: 60 outputs are ready, not 61
    with pytest.raises(ValueError, match="has not arrived"):
        O.limiter_seq(x, [(0, 100, 0, 0, 0, 37, 0)], 8000, 1.0, -1.0, True, 100)         # true peak reaches 24 further
    with pytest.raises(ValueError, match="starts after"):
        O.limiter_seq(x, [(0, 100, 500, 0, 400, 10, 0)], 8000, 1.0, -1.0, False, 100)    # output 400 reads from sample 360 on
    with pytest.raises(ValueError, match="<= 0"):
        O.limiter_seq(x, [(0, 100, 0, 0, 0, 100, 1)], 8000, 1.0, 1.0, False, 100)
    with pytest.raises(ValueError, match="look-ahead"):
        O.limiter_seq(x, [(0, 100, 0, 0, 0, 100, 1)], 50, 1.0, -1.0, False, 100)
    with pytest.raises(ValueError, match="f32"):
        O.limiter_seq(x.double(), [(0, 100, 0, 0, 0, 100, 1)], 8000, 1.0, -1.0, False, 100)
    with pytest.raises(ValueError, match="one value per sequence"):
        O.limiter_seq(x, [(0, 100, 0, 0, 0, 100, 1)], 8000, torch.ones(2), -1.0, False, 100)
    with pytest.raises(ValueError, match="outside its buffer"):
        O.true_peak_seq(x, [(0, 1001)])
    with pytest.raises(ValueError, match="device"):
        O.measure_true_peak(x)
