"""Host side of the loudness normalisation of the delivery formats (indextts_amd/output.py): the f64 restatement of
tests/loudness_ref.py against ITU-R BS.1770-4 / EBU Tech 3341 (coefficient table, the 997 Hz sine at every supported rate, both gates, the
shortest measurable sequence), the coefficients and the hop-step transition the library builds, and `AudioFormat(loudness_lufs=)` through
parsing, hashing, the stream refusals and the batcher's grouping."""
import math
import os

import numpy as np
import pytest

from indextts_amd import output as O
from tests import loudness_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_48K = ((1.53512485958697, -2.69169618940638, 1.19839281085285), (-1.69065929318241, 0.73248077421585),
             (-1.99004745483398, 0.99007225036621))


# ---- the reference against the standard -----------------------------------------------------------------------------------------------------
def test_the_48_khz_coefficients_are_the_table_of_bs_1770():
    b1, a1, b2, a2 = LR.coefficients(48000)
    assert np.max(np.abs(b1 - TABLE_48K[0])) <= 1e-12 and np.max(np.abs(a1[1:] - TABLE_48K[1])) <= 1e-12
    assert np.max(np.abs(a2[1:] - TABLE_48K[2])) <= 1e-12 and a1[0] == a2[0] == 1.0 and list(b2) == [1.0, -2.0, 1.0]
    assert LR.hop(48000) == 4800 and LR.hop(22050) == 2205 and LR.hop(11025) == 1103 and LR.hop(8000) == 800


def test_a_full_scale_997_hz_sine_reads_minus_3_01_at_48_khz():
    got = LR.loudness(LR.tone(997.0, 3.0, 48000), 48000)
    print(f"997 Hz, 0 dBFS, 48000 Hz: {got:.4f} LUFS")
    assert abs(got - (-3.01)) <= 0.005


@pytest.mark.parametrize("rate", [8000, 11025, 16000, 22050, 44100])
def test_the_sine_reads_within_the_meter_tolerance_at_every_rate(rate):
    got = LR.loudness(LR.tone(997.0, 3.0, rate), rate)
    print(f"997 Hz, 0 dBFS, {rate} Hz: {got:.4f} LUFS ({got + 3.01:+.4f})")
    assert abs(got - (-3.01)) <= 0.1                                 # EBU Tech 3341: +-0.1 LU


GATE_RATE = 22050


def _two_levels(second_dbfs):
    first = LR.tone(997.0, 2.0, GATE_RATE, -20.0)
    second = np.zeros(2 * GATE_RATE) if second_dbfs is None else LR.tone(997.0, 2.0, GATE_RATE, second_dbfs)
    return np.concatenate([first, second])


@pytest.mark.parametrize("second, kept_abs, kept", [(None, 21, 20), (-45.0, 37, 20), (-26.0, 37, 37)])
def test_gates(second, kept_abs, kept):
    """2 s at -20 dBFS, then 2 s of silence (the absolute gate drops blocks: 16 of them; the first all-silent block still holds the high-pass's
    ringing, passes it and falls to the relative gate), of -45 dBFS (the relative gate drops blocks), of -26 dBFS (neither does)"""
    m = LR.measure(_two_levels(second), GATE_RATE)
    print(f"second half {second}: {m['kept_abs']} / {m['kept']} of {m['n_blocks']} blocks, nearest block {m['margin']:.2f} LU from a gate, "
          f"{m['lufs']:.4f} LUFS")
    assert m["n_blocks"] == 37 and m["kept_abs"] == kept_abs and m["kept"] == kept
    assert m["margin"] >= 0.5
    assert math.isfinite(m["lufs"])
    alone = LR.loudness(_two_levels(None)[: 2 * GATE_RATE], GATE_RATE)      # the -20 dBFS tone by itself: -23.01
    assert abs(alone - (-23.01)) <= 0.1
    if kept == 20:                   # 17 blocks of the tone and 3 that straddle the change (3/4, 1/2, 1/4 of it): at least 18.5 / 20 of its power
        assert alone + 10.0 * math.log10(18.5 / 20.0) - 0.01 <= m["lufs"] <= alone + 0.01
    else:                            # everything counts: between the loudness of the two halves
        assert alone - 6.0 < m["lufs"] < alone


@pytest.mark.parametrize("rate", [8000, 22050])
def test_the_shortest_measurable_sequence_is_four_sub_blocks(rate):
    h = LR.hop(rate)
    x = LR.tone(997.0, (4 * h + 1) / rate, rate, -12.0)
    assert len(x) >= 4 * h + 1
    for n, blocks in ((0, 0), (4 * h - 1, 0), (4 * h, 1), (4 * h + 1, 1)):
        m = LR.measure(x[:n], rate)
        assert m["n_blocks"] == blocks
        if blocks:
            assert m["kept"] == 1 and math.isfinite(m["lufs"])
        else:
            assert m["lufs"] == -math.inf
    assert LR.loudness(x[: 4 * h], rate) == LR.loudness(x[: 4 * h + 1], rate)      # the sample past the last whole sub-block does not count


def test_gain_formula():
    assert LR.gain(-20.0, -30.0) == np.float32(10.0 ** -0.5) and LR.gain(-math.inf, -30.0) == np.float32(1.0)
    ceil_lin = np.float32(10.0 ** (-6.0 / 20.0))
    assert LR.gain(-30.0, -16.0, peak=0.5, ceiling_dbfs=-6.0) == np.float32(ceil_lin / np.float32(0.5))          # the ceiling binds
    assert LR.gain(-30.0, -16.0, peak=0.01, ceiling_dbfs=-6.0) == np.float32(10.0 ** 0.7)                         # it does not
    assert LR.gain(-30.0, -16.0, peak=0.0, ceiling_dbfs=-6.0) == np.float32(10.0 ** 0.7)


# ---- what the library builds on the host ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 11025, 22050, 48000])
def test_library_coefficients_and_transition_match_the_restatement(rate):
    from indextts_amd import _lib
    c = O.loudness_coefficients(rate)
    b1, a1, b2, a2 = LR.coefficients(rate)
    want = np.concatenate([b1, a1[1:], a2[1:]])
    assert c.shape == (23,) and np.max(np.abs(c[:7] - want)) <= 4e-16 * np.max(np.abs(want))
    phi, ref = c[7:].reshape(4, 4), LR.transition(rate)
    # A^hop by squaring against hop steps of the filters.  The entries are what is left after the state has decayed by seven orders, so the
    # two routes agree to f64 roundoff of the state's size (2^-52 per step), not of the entry's: an error of 1e-12 moves a sample by 1e-12 of
    # the state before it, six orders under the 1e-6 LU the kernels are held to
    assert np.max(np.abs(phi - ref)) <= 1e-12, (phi, ref)
    assert np.max(np.abs(ref)) < 1e-3                                # the state of one sub-block has all but died by the next
    L = _lib.lib()
    assert L.itts_pcm_loudness_hop(rate) == O.loudness_hop(rate) == LR.hop(rate)


def test_header_and_binding_declare_the_loudness_entries():
    import ctypes
    from indextts_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert "v13, additive: loudness" in hdr and "#define ITTS_ABI_VERSION 13" in hdr and _lib.ABI_VERSION == 13
    L = _lib.lib()
    for name, nargs in (("itts_pcm_loudness_seq_forward", 11), ("itts_pcm_loudness_gain_forward", 9), ("itts_pcm_loudness_coefficients", 2),
                        ("itts_pcm_loudness_workspace_bytes", 1), ("itts_pcm_loudness_hop", 1)):
        assert name + "(" in hdr and hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert f"#define ITTS_PCM_LOUDNESS_WS_DOUBLES {O.LOUDNESS_WS_DOUBLES}" in hdr
    assert f"#define ITTS_PCM_LOUDNESS_MIN_RATE {O.LOUDNESS_MIN_RATE}" in hdr and f"#define ITTS_PCM_LOUDNESS_MAX_RATE {O.LOUDNESS_MAX_RATE}" in hdr
    assert L.itts_pcm_loudness_workspace_bytes(10) == 10 * 8 * O.LOUDNESS_WS_DOUBLES
    # bad sizes are refused through itts_set_error before any launch (no device is touched)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.itts_pcm_loudness_seq_forward(None, None, None, None, 1, 1, 48000, 0, None, 0, None) == _lib.ERR_ARG
    assert b"pcm_loudness_seq" in L.itts_last_error()
    for n_seq, max_n, rate, total, ws_bytes in ((0, 1, 48000, 1, 512), (70000, 1, 48000, 1, 512), (1, -1, 48000, 1, 512), (1, 1, 3000, 1, 512),
                                                (1, 1, 48000, -1, 512), (1, 1, 48000, 8, 8 * 72 - 1)):
        assert L.itts_pcm_loudness_seq_forward(p, p, None, p, n_seq, max_n, rate, total, p, ws_bytes, None) == _lib.ERR_ARG, (n_seq, max_n, rate)
    assert L.itts_pcm_loudness_gain_forward(None, None, None, None, 1, -16.0, 0, 0.0, None) == _lib.ERR_ARG
    assert b"pcm_loudness_gain" in L.itts_last_error()
    for n_seq, target, has_ceiling, ceiling, peak in ((0, -16.0, 0, 0.0, None), (1, 1.0, 0, 0.0, None), (1, -71.0, 0, 0.0, None),
                                                     (1, float("nan"), 0, 0.0, None), (1, -16.0, 1, -1.0, None), (1, -16.0, 1, 1.0, p)):
        assert L.itts_pcm_loudness_gain_forward(p, peak, p, None, n_seq, target, has_ceiling, ceiling, None) == _lib.ERR_ARG, (n_seq, target)
    assert L.itts_pcm_loudness_coefficients(100, buf) == _lib.ERR_ARG and L.itts_pcm_loudness_coefficients(48000, None) == _lib.ERR_ARG


# ---- AudioFormat ----------------------------------------------------------------------------------------------------------------------------
def test_audio_format_carries_the_target_in_key_equality_and_hash():
    plain, loud = O.AudioFormat(48000, "pcm_f32le"), O.AudioFormat(48000, "pcm_f32le", loudness_lufs=-16)
    assert plain.loudness_lufs is None and loud.loudness_lufs == -16.0 and isinstance(loud.loudness_lufs, float)
    assert loud != plain and loud != O.AudioFormat(48000, "pcm_f32le", loudness_lufs=-23) and loud == O.AudioFormat(48000, "pcm_f32le", loudness_lufs=-16.0)
    assert hash(loud) == hash(O.AudioFormat(48000, "pcm_f32le", loudness_lufs=-16.0)) and len({plain, loud, O.AudioFormat(48000, "pcm_f32le", loudness_lufs=-23)}) == 3
    assert loud.key() == (48000, "pcm_f32le", 0.0, None, -16.0) and plain.key() == (48000, "pcm_f32le", 0.0, None, None)
    ceil = O.AudioFormat(8000, "mulaw", peak_dbfs=-1.0, loudness_lufs=-16)                       # with peak_dbfs: allowed, a ceiling
    assert ceil.key() == (8000, "mulaw", 0.0, -1.0, -16.0) and ceil.gain == np.float32(10.0 ** (-1.0 / 20)) and ceil != O.AudioFormat(8000, "mulaw", loudness_lufs=-16)
    with pytest.raises(AttributeError):
        loud.loudness_lufs = -20.0
    # the formats of before print as before
    assert repr(O.AudioFormat()) == "AudioFormat(sample_rate=22050, encoding='pcm_s16le', gain_db=0.0, peak_dbfs=None)"
    assert repr(O.AudioFormat(8000, "mulaw", peak_dbfs=-1.0)) == "AudioFormat(sample_rate=8000, encoding='mulaw', gain_db=0.0, peak_dbfs=-1.0)"
    assert repr(loud) == "AudioFormat(sample_rate=48000, encoding='pcm_f32le', gain_db=0.0, peak_dbfs=None, loudness_lufs=-16.0)"
    for edge in (-70.0, 0.0, -0.0):
        assert O.AudioFormat(loudness_lufs=edge).loudness_lufs == edge


def test_audio_format_dict_and_string_forms():
    d = O.AudioFormat.parse(dict(sample_rate=8000, encoding="pcm_s16le", loudness_lufs=-23, peak_dbfs=-2.0))
    assert d == O.AudioFormat(8000, "pcm_s16le", peak_dbfs=-2.0, loudness_lufs=-23.0)
    s = O.AudioFormat.parse("48000/pcm_s16le/-16lufs")
    assert s == O.AudioFormat(48000, loudness_lufs=-16.0) and O.AudioFormat.parse("-16 LUFS/48000") == s
    assert O.AudioFormat.parse("mulaw/-18.5lufs") == O.AudioFormat(encoding="mulaw", loudness_lufs=-18.5)
    assert O.AudioFormat.parse("-23lufs") == O.AudioFormat(loudness_lufs=-23.0)
    assert O.AudioFormat.parse("48000/pcm_s16le").loudness_lufs is None


@pytest.mark.parametrize("bad, match", [
    (dict(loudness_lufs=-70.5), r"\[-70, 0\]"), (dict(loudness_lufs=0.5), r"\[-70, 0\]"), (dict(loudness_lufs=float("nan")), "finite"),
    (dict(loudness_lufs=float("-inf")), "finite"), (dict(loudness_lufs="loud"), "number"), (dict(loudness_lufs=-16, gain_db=3.0), "not both"),
    (dict(loudness_lufs=-16, gain_db=3.0, peak_dbfs=-1.0), "not both"), ("48000/pcm_s16le/-16", "rate/encoding"),
    ("48000/-16lufs/-18lufs", "rate/encoding"), ("48000/pcm_s16le/-16lufs/x", "rate/encoding"), ("1lufs", r"\[-70, 0\]")])
def test_audio_format_refuses_bad_targets(bad, match):
    with pytest.raises(ValueError, match=match):
        O.AudioFormat.parse(bad)


def test_wrappers_check_their_tables_before_any_launch():
    import torch
    x = torch.zeros(100)
    for seqs in ([(0, 101)], [(-1, 5)], [(50, 51)], [(0, -1)], []):
        with pytest.raises(ValueError, match="outside its buffer"):
            O.loudness_seq(x, seqs, 8000)
    with pytest.raises(ValueError, match="rate"):
        O.loudness_seq(x, [(0, 100)], 2000)
    with pytest.raises(ValueError, match="f32"):
        O.loudness_seq(x.double(), [(0, 100)], 8000)
    with pytest.raises(ValueError, match="ceiling needs"):
        O.loudness_gain(torch.zeros(2, dtype=torch.float64), -16.0, None, -1.0)
    with pytest.raises(ValueError, match="device"):
        O.measure_loudness(x, 8000)


# ---- refusals, before any engine call ---------------------------------------------------------------------------------------------------------
def _tts():
    from tests.test_token_scores_host import _tts as build
    return build()


REQ = dict(spk_audio_prompt="a.wav", text="hello", lang="en", seed=3)
LOUD = dict(sample_rate=8000, loudness_lufs=-16.0)


def test_streams_refuse_a_loudness_target_before_any_engine_work():
    t = _tts()
    with pytest.raises(ValueError, match="loudness_lufs"):
        next(iter(t.infer_stream("a.wav", ["hello"], "en", audio_format=LOUD)))
    with pytest.raises(ValueError, match="loudness_lufs"):
        next(iter(t.infer_stream("a.wav", ["hello"], "en", audio_format="8000/mulaw/-16lufs")))
    with pytest.raises(ValueError, match="loudness_lufs"):
        t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global", audio_format=LOUD)
    sess = t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global")
    with pytest.raises(ValueError, match="loudness_lufs"):
        sess.submit(dict(REQ, audio_format=LOUD))
    with pytest.raises(ValueError, match="loudness_lufs|peak_dbfs"):                            # both fields: either refusal may fire first
        sess.submit(dict(REQ, audio_format=dict(LOUD, peak_dbfs=-1.0)))
    with pytest.raises(ValueError, match="loudness_lufs"):
        O.OutputStream(O.AudioFormat(**LOUD), 10)
    # bad targets go to the caller of the whole-request entries too, before anything runs
    with pytest.raises(ValueError, match="not both"):
        t.infer_requests([dict(REQ, audio_format=dict(loudness_lufs=-16, gain_db=1.0))], num_beams=1)
    with pytest.raises(ValueError, match=r"\[-70, 0\]"):
        t.infer_batch("a.wav", ["hello"], "en", audio_format=dict(loudness_lufs=3.0))
    with pytest.raises(ValueError, match="audio_format"):
        t.infer("a.wav", "hello", None, "en", audio_format=LOUD)
    assert not t.gpt.calls and not t.frontend.calls


def test_stream_batcher_hands_the_refusal_to_the_submitter():
    from indextts_amd.serving import StreamBatcher
    t = _tts()
    b = StreamBatcher(t, slots=2, max_mel_tokens=24, cfm_noise="global")
    try:
        with pytest.raises(ValueError, match="loudness_lufs"):
            list(b.submit(**dict(REQ, audio_format=LOUD)))
    finally:
        b.close()
    assert not t.gpt.calls and not t.frontend.calls


def test_dynamic_batcher_keeps_targets_apart_or_carries_them_per_request():
    from indextts_amd.serving import DynamicBatcher
    from tests.test_mixed_requests_host import _FakeTTS
    tts = _FakeTTS()
    b = DynamicBatcher(tts, max_batch=4, max_wait_ms=50)
    specs = ["8000/mulaw/-16lufs", dict(sample_rate=8000, encoding="mulaw", loudness_lufs=-16), "8000/mulaw/-23lufs", "8000/mulaw"]
    [f.result(timeout=10) for f in [b.submit(b"A", f"t{i}", "en", num_beams=1, audio_format=s) for i, s in enumerate(specs)]]
    b.close()
    assert sorted(b.batches) == [1, 1, 2]                            # equal targets share a batch however they were spelled; others do not
    by_size = {len(c[1]): c[2] for c in tts.batch_calls}
    assert by_size[2] == {"num_beams": 1, "audio_format": O.AudioFormat(8000, "mulaw", loudness_lufs=-16.0)}
    assert sorted(c[2]["audio_format"].loudness_lufs or 0.0 for c in tts.batch_calls if len(c[1]) == 1) == [-23.0, 0.0]
    tts = _FakeTTS()
    b = DynamicBatcher(tts, max_batch=4, max_wait_ms=2000, mixed=True)
    futs = [b.submit(b"A", f"t{i}", "en", num_beams=1, audio_format=s) for i, s in enumerate(specs)]
    [f.result(timeout=10) for f in futs]
    with pytest.raises(ValueError, match="not both"):
        b.submit(b"A", "t", "en", audio_format=dict(loudness_lufs=-16, gain_db=2.0))       # refused at submit: the error is the caller's
    b.close()
    (reqs, defaults), = tts.request_calls                            # mixed: ONE batch, the target travels with its request
    assert defaults == {"num_beams": 1}
    assert [r["audio_format"].loudness_lufs for r in reqs] == [-16.0, -16.0, -23.0, None]
