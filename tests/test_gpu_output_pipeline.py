"""`audio_format=` through the pipeline entries on the real HIP engines (the tiny models of tests/test_gpu_stream_session.py): a formatted
request is bit for bit `output.convert` of its own 22050 Hz float rows, an unformatted one in the same batch is untouched, a stream with a format
gets the bytes of `infer_stream` over the request alone in any slot and at any `poll_steps`, its pieces concatenate to the one-shot conversion,
and `AudioFormat()` stays within 1 LSB of the legacy int16 path."""
import numpy as np
import pytest
import torch

from indextts_amd import output as O
from tests import pcm_ref as R
from tests.test_gpu_cfm_noise_pipeline import VoiceFrontend
from tests.test_gpu_pipeline import _s2_engines, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SRC = 22050
CHUNK, OVERLAP, MAX_TEXT = 8, 2, 30
SESSION = dict(chunk_size=CHUNK, overlap_size=OVERLAP, max_mel_tokens=24, max_text_tokens_per_segment=MAX_TEXT)
KW = dict(num_beams=1, max_mel_tokens=24, cfm_noise="request", interval_silence=40)

REQUESTS = [
    dict(spk_audio_prompt="alice.wav", text="hello world. and a second sentence", lang="en", seed=11),
    dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=12, temperature=1.1, top_k=12),
    dict(spk_audio_prompt="carol.wav", text="a much longer second sentence here. ok", lang="en", seed=13),
]
FORMATS = ["48000/pcm_f32le", "8000/mulaw", None]
STREAMS = [
    dict(spk_audio_prompt="alice.wav", text="hello world", lang="en", seed=11, max_mel_tokens=5, audio_format="8000/mulaw"),
    dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=12, max_mel_tokens=14, temperature=1.1, top_k=12,
         audio_format=dict(sample_rate=48000, encoding="pcm_s16le", gain_db=-3.0)),
    dict(spk_audio_prompt="carol.wav", text="a much longer second sentence", lang="en", seed=13, max_mel_tokens=20),
    dict(spk_audio_prompt="alice.wav", text="one more for the first voice", lang="en", seed=14, max_mel_tokens=24, duration_factor=1.25,
         audio_format="16000/alaw"),
    dict(spk_audio_prompt="bob.wav", text="and the last one", lang="en", seed=15, max_mel_tokens=17, audio_format="8000/mulaw"),
]


@pytest.fixture(scope="module")
def tts():
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    t.semantic_codec, t.s2mel = _s2_engines("fp32")[:2]
    return t


def _with(reqs, formats):
    return [dict(r, audio_format=f) if f is not None else dict(r) for r, f in zip(reqs, formats)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_infer_requests_delivers_each_request_in_its_own_format(tts):
    plain = tts.infer_requests(REQUESTS, **KW)
    floats = tts.infer_requests(REQUESTS, audio_format="22050/pcm_f32le", **KW)
    mixed = tts.infer_requests(_with(REQUESTS, FORMATS), **KW)
    for (sr, w), (sr0, w0) in zip(floats, plain):                    # the 22050 Hz float rows: the legacy int16 is their truncation
        assert sr == sr0 == SRC and w.dtype == np.float32 and w.shape == w0.shape and w.ndim == 2 and np.abs(w).max() > 0
        assert np.abs(np.clip(w * 32767.0, -32767, 32767) - w0).max() <= 1.0
    assert np.array_equal(mixed[2][1], plain[2][1]) and mixed[2][0] == SRC and mixed[2][1].dtype == np.int16      # untouched by its batch mates
    for r, spec in enumerate(FORMATS[:2]):
        fmt = O.AudioFormat.parse(spec)
        L, M, H, K = R.params(SRC, fmt.sample_rate)
        sr, w = mixed[r]
        own, = O.convert([_dev(floats[r][1][:, 0])], None, [[0]], fmt)
        assert sr == fmt.sample_rate and w.dtype == fmt.dtype and w.shape == (R.out_len(floats[r][1].shape[0], L, M), 1)
        assert np.array_equal(w[:, 0].view(np.uint8), own.view(np.uint8)), spec
    assert not np.all(mixed[0][1] == 0) and len(set(mixed[1][1][:, 0].tolist())) > 4
    n_sil = int(SRC * 40 / 1000.0)                                    # request 0 has two segments: the silence between them is there at 22050 Hz
    assert plain[0][1].shape[0] > n_sil and np.any(np.all(np.lib.stride_tricks.sliding_window_view(floats[0][1][:, 0], n_sil) == 0, axis=1))
    # the call-wide default, and a request key over it
    again = tts.infer_requests(_with(REQUESTS, [None, "8000/mulaw", None]), audio_format="48000/pcm_f32le", **KW)
    assert np.array_equal(again[0][1], mixed[0][1]) and np.array_equal(again[1][1], mixed[1][1]) and again[2][0] == 48000
    # the default format runs the new path: within 1 LSB of the legacy result, same shape
    default = tts.infer_requests(REQUESTS, audio_format=O.AudioFormat(), **KW)
    for (sr, w), (_, w0) in zip(default, plain):
        assert sr == SRC and w.dtype == np.int16 and w.shape == w0.shape
        assert np.abs(w.astype(np.int32) - w0.astype(np.int32)).max() <= 1
    # peak normalisation sees the whole request
    (sr, w), = tts.infer_requests([dict(REQUESTS[0], audio_format=dict(sample_rate=16000, encoding="pcm_f32le", peak_dbfs=-6.0))], **KW)
    assert sr == 16000 and abs(float(np.abs(w).max()) - 10.0 ** (-6.0 / 20)) <= 1e-6


def test_infer_batch_takes_the_format(tts):
    texts = ["hello world. and a second sentence", "ok"]
    kw = dict(num_beams=1, max_mel_tokens=24, cfm_noise="request", seed=5, interval_silence=40)
    plain = tts.infer_batch("alice.wav", texts, "en", **kw)
    floats = tts.infer_batch("alice.wav", texts, "en", audio_format="22050/pcm_f32le", **kw)
    got = tts.infer_batch("alice.wav", texts, "en", audio_format="8000/alaw", **kw)
    for (sr, w), (_, f), (_, w0) in zip(got, floats, plain):
        own, = O.convert([_dev(f[:, 0])], None, [[0]], "8000/alaw")
        assert sr == 8000 and w.dtype == np.uint8 and np.array_equal(w[:, 0], own) and f.shape == w0.shape
        assert np.abs(np.clip(f * 32767.0, -32767, 32767) - w0).max() <= 1.0


# ---- streams --------------------------------------------------------------------------------------------------------------------------------
def run_alone(tts, req):
    r = dict(req)
    gen = tts.infer_stream(r.pop("spk_audio_prompt"), [r.pop("text")], r.pop("lang"), chunk_size=CHUNK, overlap_size=OVERLAP,
                           max_text_tokens_per_segment=MAX_TEXT, cfm_noise="request", **r)
    return [(sr, audio[0], bool(done[0]), k) for k, (sr, audio, done) in enumerate(gen)]


def drain(sess):
    out, n = {}, 0
    while sess.active:
        for sid, sr, piece, done, k in sess.step():
            out.setdefault(sid, []).append((sr, piece, done, k))
        n += 1
        assert n < 400
    return out


@pytest.fixture(scope="module")
def alone(tts):
    return [run_alone(tts, r) for r in STREAMS]


def test_alone_streams_carry_their_format_and_concatenate_to_the_one_shot_conversion(tts, alone):
    for req, ev in zip(STREAMS, alone):
        fmt = O.AudioFormat.parse(req.get("audio_format"))
        assert ev and ev[-1][2] and all(p is not None for _, p, _, _ in ev)
        if fmt is None:
            assert all(sr == SRC and p.dtype == np.int16 for sr, p, _, _ in ev)
            continue
        assert all(sr == fmt.sample_rate and p.dtype == fmt.dtype and p.ndim == 1 for sr, p, _, _ in ev)
        floats = run_alone(tts, dict(req, audio_format="22050/pcm_f32le"))
        assert [(d, k) for _, _, d, k in floats] == [(d, k) for _, _, d, k in ev]
        whole = np.concatenate([p for _, p, _, _ in floats])
        one_shot, = O.convert([_dev(whole)], None, [[0]], fmt)
        cat = np.concatenate([p for _, p, _, _ in ev])
        L, M, _, _ = R.params(SRC, fmt.sample_rate)
        assert len(cat) == R.out_len(len(whole), L, M) and np.array_equal(cat, one_shot), req["audio_format"]


@pytest.mark.parametrize("slots, poll_steps", [(2, 8), (3, 3)])
def test_session_streams_are_bit_equal_to_the_request_alone(tts, alone, slots, poll_steps):
    with tts.stream_session(slots=slots, poll_steps=poll_steps, **SESSION) as sess:
        ids = [sess.submit(r) for r in STREAMS]                       # three formats and a stream without one share the session
        with pytest.raises(ValueError, match="peak_dbfs"):
            sess.submit(dict(STREAMS[0], audio_format=dict(sample_rate=8000, peak_dbfs=-1.0)))
        out = drain(sess)
    for i, sid in enumerate(ids):
        got, ref = out[sid], alone[i]
        assert [(sr, d, k) for sr, _, d, k in got] == [(sr, d, k) for sr, _, d, k in ref], i
        for (_, p, _, k), (_, p0, _, _) in zip(got, ref):
            assert p.dtype == p0.dtype and p.shape == p0.shape and np.array_equal(p, p0), (i, k)


def test_default_format_stream_is_within_one_lsb_of_the_legacy_stream(tts, alone):
    req = {k: v for k, v in STREAMS[3].items() if k != "audio_format"}
    legacy = run_alone(tts, req)
    new = run_alone(tts, dict(req, audio_format=O.AudioFormat()))
    with tts.stream_session(slots=2, audio_format=O.AudioFormat(), **SESSION) as sess:      # the session default
        sid = sess.submit(req)
        in_session = drain(sess)[sid]
    assert len(legacy) == len(new) == len(in_session) >= 2
    for (sr0, p0, d0, k0), (sr, p, d, k), (_, q, _, _) in zip(legacy, new, in_session):
        assert (sr, d, k) == (sr0, d0, k0) and p.dtype == np.int16 and p.shape == p0.shape and np.array_equal(p, q)
        assert np.abs(p.astype(np.int32) - p0.astype(np.int32)).max() <= 1
