"""Host side of the delivery formats (indextts_amd/output.py): the resampler design's frequency response, the f64
restatement of tests/pcm_ref.py against independent references (scipy's upfirdn, CPython's audioop), the streaming arithmetic, AudioFormat,
the WAV writer, the ABI declarations, and every refusal -- before any engine call."""
import os
import struct

import numpy as np
import pytest
import torch

from indextts_amd import output as O
from tests import pcm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = 22050


# ---- the design -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", R.RATES)
def test_prototype_response_meets_the_16_bit_floor(rate):
    """|H(f)| / L of the f32-rounded prototype, in f64: flat within 0.001 dB up to 0.85 of the lower Nyquist, at most -96 dB from 1.15 of it
    upward -- so what aliases below the passband edge stays under the 16-bit floor (Z = 24, beta = 10 measure 0.00009 dB and -100.7 dB)."""
    L, M, H, K = R.params(SRC, rate)
    h = R.prototype_f32(SRC, rate)
    fs_hi, nyq = SRC * L, min(SRC, rate) / 2
    nfft = 1 << 22
    mag = np.abs(np.fft.rfft(h, nfft)) / L
    f = np.arange(mag.size) * (fs_hi / nfft)
    ripple = float(np.max(np.abs(20 * np.log10(mag[f <= 0.85 * nyq]))))
    stop = float(20 * np.log10(np.max(mag[f >= 1.15 * nyq])))
    table = O.phase_table(SRC, rate).astype(np.float64)
    dc = table.sum(axis=0)
    print(f"{SRC} -> {rate}: L {L} M {M} H {H} K {K}; passband ripple {ripple:.6f} dB, stopband {stop:.2f} dB, "
          f"per-phase DC gain {dc.min():.9f} .. {dc.max():.9f} (spread {dc.max() - dc.min():.3e})")
    assert ripple <= 0.001 and stop <= -96.0
    assert K * L * 4 <= O.TABLE_MAX_BYTES and O.rate_supported(SRC, rate)


@pytest.mark.parametrize("rate", R.RATES)
def test_parameters_prototype_and_table_layout(rate):
    L, M, H, K = R.params(SRC, rate)
    assert O.resample_params(SRC, rate) == (L, M, H, K)
    assert np.array_equal(O.prototype(SRC, rate), R.prototype(SRC, rate))
    h32, table = R.prototype(SRC, rate).astype(np.float32), O.phase_table(SRC, rate)
    assert table.shape == (K, L) and table.dtype == np.float32
    for r in sorted({0, min(1, L - 1), L // 2, L - 1}):                          # each residue's column lists its support's coefficients in input order
        m = r + L * (H // L + 2)                                     # far enough in for the whole support to exist
        idx = list(R.support(m, 10 ** 9, L, M, H))
        want = np.zeros(K, dtype=np.float32)
        want[: len(idx)] = [h32[m * M - i * L + H] for i in idx]
        assert len(idx) in (K, K - 1) and np.array_equal(table[:, r], want), r


def test_rates_outside_the_table_budget_are_refused():
    assert O.rate_supported(SRC, SRC) and O.rate_supported(48000, 8000)
    assert not O.rate_supported(SRC, 22051)
    with pytest.raises(ValueError, match="not supported"):
        O.AudioFormat(sample_rate=22051)
    with pytest.raises(ValueError, match="coefficient table"):
        O.resample_table(SRC, 22051, "cpu")


# ---- the restatement against independent references -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", R.RATES)
def test_restatement_equals_scipy_upfirdn(rate):
    sig = pytest.importorskip("scipy.signal")
    L, M, H, K = R.params(SRC, rate)
    h = R.prototype_f32(SRC, rate)
    x = np.random.default_rng(rate).standard_normal(3 * K + 5)
    pad = (-H) % M                                                   # leading zeros so that the centre tap sits on a multiple of M
    full = sig.upfirdn(np.concatenate([np.zeros(pad), h]), x, up=L, down=M)
    first = (H + pad) // M
    y, mag = R.resample(x, SRC, rate, h)
    assert len(y) == R.out_len(len(x), L, M)
    assert np.max(np.abs(full[first: first + len(y)] - y)) <= 1e-12 * max(1.0, float(mag.max()))


def test_g711_restatement_equals_audioop_on_every_sample():
    audioop = pytest.importorskip("audioop")
    q = np.arange(-32768, 32768, dtype=np.int16)
    raw = q.astype("<i2").tobytes()
    assert np.array_equal(R.g711(q, "mulaw"), np.frombuffer(audioop.lin2ulaw(raw, 2), dtype=np.uint8))
    assert np.array_equal(R.g711(q, "alaw"), np.frombuffer(audioop.lin2alaw(raw, 2), dtype=np.uint8))


def test_s16_rounds_half_to_even_and_clamps():
    x = np.array([0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767, -1.5 / 32767, 1.5, -1.5, np.nan, np.inf, -np.inf], dtype=np.float32)
    q = R.encode_s16(x)
    assert q[-5:].tolist() == [32767, -32767, 0, 32767, -32767]
    exact = x[:5].astype(np.float32) * np.float32(32767)             # whatever the f32 product is, it is rounded half to even
    assert q[:5].tolist() == [int(np.rint(float(v))) for v in exact]
    assert R.encode_f32(x)[-5:].tolist() == [1.0, -1.0, 0.0, 1.0, -1.0]


# ---- streaming arithmetic -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.SPLITS)
@pytest.mark.parametrize("rate", R.RATES)
def test_stream_pieces_tile_the_output_and_the_carry_keeps_every_needed_sample(rate, kind):
    L, M, H, K = O.resample_params(SRC, rate)
    N = 3 * K + 611
    rng = np.random.default_rng(7)
    pieces = R.splits(kind, N, rng)
    assert sum(pieces) == N and (kind != "empty_final" or pieces[-1] == 0)
    n_in = n_out = 0
    mine = []
    carry_from = 0                                              # the stream's first sample still held
    for k, p in enumerate(pieces):
        final = k == len(pieces) - 1
        in_off = carry_from
        n_in += p
        ready = O.outputs_ready(n_in, final, L, M, H)
        assert ready >= n_out and ready == R.ready(n_in, final, L, M, H)
        for m in {n_out, ready - 1} if ready > n_out else ():       # supports are monotone in m: the ends of the piece's range bound them all
            sup = R.support(m, 10 ** 12, L, M, H)
            assert sup[0] >= in_off, "the carry dropped a sample this piece needs"
            assert final or sup[-1] < n_in, "a non-final piece reads a sample that has not arrived"
        if not final:                                                # and nothing more could have been produced
            assert R.support(ready, 10 ** 12, L, M, H)[-1] >= n_in
        carry_from = O.first_needed(ready, n_in, L, M, H)
        mine.append((n_in, n_out, ready - n_out, carry_from))
        n_out = ready
        assert in_off <= carry_from <= n_in
        assert n_in - carry_from <= K + 1, "the carry is the filter's span, not the stream"
    assert n_out == -(-N * L // M) == O.resampled_length(N, L, M)   # the ranges [previous ready, ready) tile [0, ceil(N L / M)) in order
    assert mine == R.stream_schedule(pieces, L, M, H)


def test_piece_plan_matches_rowstream_lengths():
    from indextts_amd.streaming import RowStream
    for chunk, lasts in (([3000, 2800, 2600], [False, False, True]), ([3000, 900], [False, True]), ([700], [True]), ([3000, 2800], [False, False])):
        row = RowStream(10, 2, 1.0)
        ovlp, tail = row.ovlp, None
        assert ovlp == 512
        for a, last in zip(chunk, lasts):
            plan = O.piece_plan(None if tail is None else tail, a, ovlp, last)
            got = row.push(np.zeros(a, dtype=np.float32), last)
            assert len(got) == plan["piece_len"] and (0 if row.tail is None else len(row.tail)) == plan["keep_len"]
            tail = None if last else plan["keep_len"]
    short = O.piece_plan(512, 300, 512, False)                       # a chunk shorter than the overlap: blended over what it has, nothing held back
    assert short["n_blend"] == 300 and short["piece_len"] == 300 and short["keep_len"] == 0


# ---- AudioFormat ----------------------------------------------------------------------------------------------------------------------------
def test_audio_format_defaults_parsing_and_hash():
    f = O.AudioFormat()
    assert (f.sample_rate, f.encoding, f.gain_db, f.peak_dbfs) == (22050, "pcm_s16le", 0.0, None) and f.dtype is np.int16
    assert O.AudioFormat.parse(None) is None and O.AudioFormat.parse(f) is f
    m = O.AudioFormat.parse("8000/mulaw")
    assert m == O.AudioFormat(8000, "mulaw") and hash(m) == hash(O.AudioFormat(8000, "mulaw")) and m.dtype is np.uint8
    assert O.AudioFormat.parse("mulaw/8000") == m and O.AudioFormat.parse("48000") == O.AudioFormat(48000)
    assert O.AudioFormat.parse("pcm_f32le") == O.AudioFormat(encoding="pcm_f32le")
    d = O.AudioFormat.parse(dict(sample_rate=48000, encoding="pcm_f32le", peak_dbfs=-1.0))
    assert d.peak_dbfs == -1.0 and d.dtype is np.float32 and d != O.AudioFormat(48000, "pcm_f32le") and len({d, m, f, O.AudioFormat()}) == 3
    assert d.gain == np.float32(10.0 ** (-1.0 / 20)) and O.AudioFormat(gain_db=6.0).gain == np.float32(10.0 ** 0.3)
    with pytest.raises(AttributeError):
        f.sample_rate = 8000
    for rate in R.RATES + (22050,):
        assert O.AudioFormat(rate).sample_rate == rate


@pytest.mark.parametrize("bad, match", [
    (dict(sample_rate=0), "positive integer"), (dict(sample_rate=8000.0), "positive integer"), (dict(sample_rate=True), "positive integer"),
    (dict(encoding="mp3"), "encoding"), (dict(gain_db=float("nan")), "finite"), (dict(gain_db="loud"), "numbers"),
    (dict(peak_dbfs=1.0), "<= 0"), (dict(gain_db=3.0, peak_dbfs=-1.0), "not both"), (dict(bitrate=64), "unknown keys"),
    ("8000/mulaw/x", "rate/encoding"), ("8000/16000", "rate/encoding"), ("", "rate/encoding"), (8000, "expected an AudioFormat")])
def test_audio_format_refuses(bad, match):
    with pytest.raises(ValueError, match=match):
        O.AudioFormat.parse(bad)


# ---- WAV ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec, tag, width", [("22050/pcm_s16le", 1, 2), ("48000/pcm_f32le", 3, 4), ("8000/alaw", 6, 1), ("8000/mulaw", 7, 1)])
def test_wav_header_per_format_tag(tmp_path, spec, tag, width):
    fmt = O.AudioFormat.parse(spec)
    data = (np.arange(101) % 50).astype(fmt.dtype)                   # an odd byte count for the one-byte encodings: the data chunk is padded
    path = str(tmp_path / "a.wav")
    O.save_audio_wav(path, data, fmt)
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:12] == b"WAVE" and struct.unpack("<I", raw[4:8])[0] == len(raw) - 8
    pos, chunks = 12, {}
    while pos < len(raw):
        cid, size = raw[pos: pos + 4], struct.unpack("<I", raw[pos + 4: pos + 8])[0]
        chunks[cid] = raw[pos + 8: pos + 8 + size]
        pos += 8 + size + (size & 1)
    assert pos == len(raw)
    got_tag, ch, sr, byte_rate, align, bits = struct.unpack("<HHIIHH", chunks[b"fmt "][:16])
    assert (got_tag, ch, sr, byte_rate, align, bits) == (tag, 1, fmt.sample_rate, fmt.sample_rate * width, width, 8 * width)
    if tag == 1:
        assert len(chunks[b"fmt "]) == 16 and b"fact" not in chunks
    else:
        assert len(chunks[b"fmt "]) == 18 and struct.unpack("<I", chunks[b"fact"])[0] == 101
    assert chunks[b"data"] == data.astype(data.dtype.newbyteorder("<")).tobytes()
    with pytest.raises(ValueError, match="data is"):
        O.save_audio_wav(path, data.astype(np.float64), fmt)
    if tag == 1:                                                     # the standard library reads the PCM file back
        import wave
        with wave.open(path, "rb") as w:
            assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 2, 22050, 101)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_delivery_entries():
    from indextts_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert "v13, additive: delivery formats" in hdr and "#define ITTS_ABI_VERSION 13" in hdr and _lib.ABI_VERSION == 13
    L = _lib.lib()
    for name, nargs in (("itts_pcm_resample_seq_forward", 11), ("itts_pcm_peak_seq_forward", 6), ("itts_pcm_encode_seq_forward", 9),
                        ("itts_pcm_stream_piece_seq_forward", 10), ("itts_pcm_resample_tile", 0)):
        assert name + "(" in hdr and hasattr(L, name) and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert L.itts_pcm_resample_tile() == O.RESAMPLE_TILE == 1024 and "#define ITTS_PCM_RESAMPLE_TILE 1024" in hdr
    for enc, code in O.ENCODINGS.items():
        assert f"#define ITTS_PCM_{enc.replace('pcm_', '').upper()} {code}" in hdr
    # bad sizes are refused through itts_set_error before any launch (no device is touched)
    assert L.itts_pcm_resample_seq_forward(None, None, None, None, 1, 1, 1, 1, 1, 3, None) == _lib.ERR_ARG
    assert b"pcm_resample_seq" in L.itts_last_error()
    assert L.itts_pcm_peak_seq_forward(None, None, None, 0, 0, None) == _lib.ERR_ARG
    assert L.itts_pcm_encode_seq_forward(None, None, None, 1, 1, 9, None, None, None) == _lib.ERR_ARG
    assert L.itts_pcm_stream_piece_seq_forward(None, None, None, None, None, None, None, 1, 1, None) == _lib.ERR_ARG


# ---- refusals, before any engine call -------------------------------------------------------------------------------------------------------
def _tts():
    from tests.test_token_scores_host import _tts as build
    return build()


REQ = dict(spk_audio_prompt="a.wav", text="hello", lang="en", seed=3)


def test_bad_formats_and_unsupported_entries_are_refused_before_any_engine_work():
    t = _tts()
    with pytest.raises(ValueError, match="encoding"):
        t.infer_requests([dict(REQ, audio_format="8000/mp3")], num_beams=1)
    with pytest.raises(ValueError, match="encoding"):
        t.infer_requests([REQ], num_beams=1, audio_format="8000/mp3")
    with pytest.raises(ValueError, match="not both"):
        t.infer_batch("a.wav", ["hello"], "en", audio_format=dict(gain_db=1.0, peak_dbfs=-3.0))
    with pytest.raises(ValueError, match="encoding"):
        next(iter(t.infer_stream("a.wav", ["hello"], "en", audio_format="8000/mp3")))
    with pytest.raises(ValueError, match="peak_dbfs"):
        next(iter(t.infer_stream("a.wav", ["hello"], "en", audio_format=dict(peak_dbfs=-1.0))))
    with pytest.raises(ValueError, match="peak_dbfs"):
        t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global", audio_format=dict(peak_dbfs=-1.0))
    sess = t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global")
    with pytest.raises(ValueError, match="peak_dbfs"):
        sess.submit(dict(REQ, audio_format=dict(sample_rate=8000, peak_dbfs=-1.0)))
    with pytest.raises(ValueError, match="encoding"):
        sess.submit(dict(REQ, audio_format="8000/mp3"))
    with pytest.raises(ValueError, match="audio_format"):
        t.infer("a.wav", "hello", None, "en", audio_format="8000/mulaw")
    with pytest.raises(ValueError, match="audio_format"):
        next(iter(t.infer_generator("a.wav", "hello", None, "en", audio_format="8000/mulaw")))
    assert not t.gpt.calls and not t.frontend.calls


def test_distributed_and_older_pipelines_refuse_audio_format():
    from indextts_amd import dist as D
    from indextts_amd.infer import IndexTTS
    from indextts_amd.infer_v2 import IndexTTS2 as V2
    t = _tts()
    world = D.world
    D.world = lambda: 2
    try:
        with pytest.raises(ValueError, match="audio_format"):
            t.infer_batch("a.wav", ["hello"], "en", audio_format="8000/mulaw")
    finally:
        D.world = world
    v2 = object.__new__(V2)
    with pytest.raises(ValueError, match="audio_format"):
        v2.infer("a.wav", "hello", None, audio_format="8000/mulaw")
    with pytest.raises(ValueError, match="audio_format"):
        next(iter(v2.infer_stream("a.wav", ["hello"], audio_format="8000/mulaw")))
    with pytest.raises(ValueError, match="audio_format"):
        v2.infer_requests([REQ], audio_format="8000/mulaw")
    with pytest.raises(ValueError, match="audio_format"):
        v2.infer_requests([dict(REQ, audio_format="8000/mulaw")])
    with pytest.raises(ValueError, match="audio_format"):
        v2.infer_batch("a.wav", ["hello"], None, audio_format="8000/mulaw")
    with pytest.raises(ValueError, match="audio_format"):
        v2.stream_session(slots=2, audio_format="8000/mulaw")
    with pytest.raises(ValueError, match="audio_format"):
        IndexTTS._gen_kwargs(dict(audio_format="8000/mulaw"))
    assert not t.gpt.calls and not t.frontend.calls


def test_without_audio_format_the_entries_return_what_they_returned():
    t = _tts()
    (sr, wav), = t.infer_requests([REQ], num_beams=1, max_mel_tokens=24)
    assert sr == 22050 and wav.dtype == np.int16 and wav.ndim == 2 and wav.shape[1] == 1
    assert "audio_format" not in t.gpt.calls[-1][2]


def test_dynamic_batcher_keys_groups_by_format_or_carries_it_per_request():
    from indextts_amd.serving import DynamicBatcher
    from tests.test_mixed_requests_host import _FakeTTS
    tts = _FakeTTS()
    b = DynamicBatcher(tts, max_batch=4, max_wait_ms=50)
    specs = ["8000/mulaw", dict(sample_rate=8000, encoding="mulaw"), None, "48000/pcm_f32le"]
    [f.result(timeout=10) for f in [b.submit(b"A", f"t{i}", "en", num_beams=1, audio_format=s) for i, s in enumerate(specs)]]
    b.close()
    assert sorted(b.batches) == [1, 1, 2]                            # equal formats share a batch however they were spelled; others do not
    by_size = {len(c[1]): c[2] for c in tts.batch_calls}
    assert by_size[2] == {"num_beams": 1, "audio_format": O.AudioFormat(8000, "mulaw")}
    assert sorted(str(c[2].get("audio_format")) for c in tts.batch_calls if len(c[1]) == 1) == sorted(["None", str(O.AudioFormat(48000, "pcm_f32le"))])
    tts = _FakeTTS()
    b = DynamicBatcher(tts, max_batch=4, max_wait_ms=2000, mixed=True)
    futs = [b.submit(b"A", f"t{i}", "en", num_beams=1, audio_format=s) for i, s in enumerate(specs)]
    [f.result(timeout=10) for f in futs]
    with pytest.raises(ValueError, match="encoding"):
        b.submit(b"A", "t", "en", audio_format="8000/mp3")           # refused at submit: the error is the caller's, not the batch's
    b.close()
    (reqs, defaults), = tts.request_calls                            # mixed: ONE batch, the format travels with its request
    assert defaults == {"num_beams": 1}
    assert [r.get("audio_format") for r in reqs] == [O.AudioFormat(8000, "mulaw")] * 2 + [None, O.AudioFormat(48000, "pcm_f32le")]


def test_synthesize_tasks_passes_the_format_and_writes_its_wave_tag(tmp_path):
    from indextts_amd.serving import synthesize_tasks

    class TTS:
        def __init__(self):
            self.calls = []

        def infer_batch(self, spk, texts, lang, emo_audio_prompt=None, emo_alpha=1.0, **gen):
            self.calls.append(dict(gen))
            fmt = O.AudioFormat.parse(gen.get("audio_format"))
            if fmt is None:
                return [(22050, np.full((30, 1), 100, dtype=np.int16)) for _ in texts]
            return [(fmt.sample_rate, np.full((30, 1), 7, dtype=fmt.dtype)) for _ in texts]

    tts = TTS()
    tasks = [dict(voice_path="v.wav", text="a", output_path=str(tmp_path / "a.wav")), dict(voice_path="v.wav", text="b", output_path=str(tmp_path / "b.wav"))]
    synthesize_tasks(tts, tasks, lang="en", audio_format="8000/mulaw")
    assert tts.calls == [{"audio_format": "8000/mulaw"}]
    raw = open(tasks[0]["output_path"], "rb").read()
    assert struct.unpack("<HHI", raw[20:28]) == (7, 1, 8000) and raw[-30:] == bytes([7]) * 30
    synthesize_tasks(tts, tasks, lang="en")                          # no format: the 16-bit PCM writer, as always
    raw = open(tasks[0]["output_path"], "rb").read()
    assert struct.unpack("<HHI", raw[20:28]) == (1, 1, 22050) and tts.calls[-1] == {}
