"""`audio_format=` with `limit_dbfs` / `true_peak` through the pipeline entries on the real HIP engines (the tiny models of
tests/test_gpu_output_pipeline.py): requests without the new fields keep their bytes beside one with them, a loudness target and a ceiling are
both met, `last_limiter` is filled, a stream with a limiter never exceeds its ceiling and gets in a session the bytes it gets alone, and a
true-peak target is met as `measure_true_peak` reads the delivered samples."""
import math

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
U = 2.0 ** -24
CHUNK, OVERLAP, MAX_TEXT = 8, 2, 30
SESSION = dict(chunk_size=CHUNK, overlap_size=OVERLAP, max_mel_tokens=24, max_text_tokens_per_segment=MAX_TEXT)
KW = dict(num_beams=1, max_mel_tokens=24, cfm_noise="request", interval_silence=40)

LIMITED = dict(sample_rate=48000, encoding="pcm_f32le", loudness_lufs=-16.0, limit_dbfs=-1.0)
A = dict(spk_audio_prompt="alice.wav", text="hello world. and a second sentence", lang="en", seed=11, audio_format=LIMITED)
B = dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=12, temperature=1.1, top_k=12, audio_format="8000/mulaw")
C = dict(spk_audio_prompt="carol.wav", text="a much longer second sentence here. ok", lang="en", seed=13)
STREAMS = [
    dict(spk_audio_prompt="alice.wav", text="hello world", lang="en", seed=11, max_mel_tokens=14,
         audio_format=dict(sample_rate=16000, encoding="pcm_f32le", gain_db=12.0, limit_dbfs=-1.0)),
    dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=12, max_mel_tokens=20, temperature=1.1, top_k=12,
         audio_format="22050/pcm_s16le/-3limit/tp"),
    dict(spk_audio_prompt="carol.wav", text="a much longer second sentence", lang="en", seed=13, max_mel_tokens=17, audio_format="8000/mulaw"),
    dict(spk_audio_prompt="alice.wav", text="one more for the first voice", lang="en", seed=14, max_mel_tokens=24,
         audio_format=dict(sample_rate=8000, encoding="mulaw", gain_db=12.0, limit_dbfs=-6.0)),
]


@pytest.fixture(scope="module")
def tts():
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    t.semantic_codec, t.s2mel = _s2_engines("fp32")[:2]
    return t


@pytest.fixture(scope="module")
def batch(tts):
    out = tts.infer_requests([A, B, C], **KW)
    return out, list(tts.last_limiter), list(tts.last_loudness)


def _fmt(req, fmt):
    return dict({k: v for k, v in req.items() if k != "audio_format"}, audio_format=fmt)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_requests_without_the_new_fields_keep_their_bytes_beside_one_with_them(tts, batch):
    (_, out_b, out_c), lim, _ = batch
    (alone_b, alone_c) = tts.infer_requests([B, C], **KW)
    assert tts.last_limiter == [None, None]
    assert out_c[0] == alone_c[0] == SRC and out_c[1].dtype == np.int16 and np.array_equal(out_c[1], alone_c[1])
    assert out_b[0] == alone_b[0] == 8000 and out_b[1].dtype == np.uint8 and np.array_equal(out_b[1], alone_b[1])
    assert isinstance(lim[0], dict) and lim[1] is None and lim[2] is None


def test_a_loudness_target_and_a_ceiling_are_both_met(tts, batch):
    (out_a, _, _), lim, loud = batch
    c = O.AudioFormat.parse(LIMITED).ceiling
    sr, w = out_a
    assert sr == 48000 and w.dtype == np.float32 and np.abs(w).max() <= c                     # the ceiling: an exact f32 compare
    tts.infer_requests([_fmt(A, dict(LIMITED, limit_dbfs=None))], **KW)                       # the target alone: the unceilinged gain
    free, = tts.last_loudness
    (_, w_peak), = tts.infer_requests([_fmt(A, dict(LIMITED, limit_dbfs=None, peak_dbfs=-1.0))], **KW)      # the static ceiling of before
    static, = tts.last_loudness
    print(f"-16 LUFS: measured {loud[0]['measured_lufs']:.4f}; gain {loud[0]['gain_db']:.4f} dB with the limiter, {static['gain_db']:.4f} dB with "
          f"peak_dbfs; unceilinged peak {free['peak_dbfs_after']:.4f} dBFS; limiter {lim[0]}")
    assert loud[0]["gain_db"] == free["gain_db"] and loud[0]["measured_lufs"] == free["measured_lufs"] == static["measured_lufs"]
    assert static["gain_db"] <= loud[0]["gain_db"] and (static["gain_db"] < loud[0]["gain_db"]) == (free["peak_dbfs_after"] > -1.0)
    assert (lim[0]["max_reduction_db"] > 0.0) == (free["peak_dbfs_after"] > -1.0) and np.abs(w_peak).max() <= c + 2e-7
    # a target no signal reaches under its ceiling (0 LUFS with peaks 12 dB under full scale): the static ceiling costs loudness, the limiter none
    hot = dict(sample_rate=16000, encoding="pcm_f32le", loudness_lufs=0.0)
    (sr, w), = tts.infer_requests([_fmt(A, dict(hot, limit_dbfs=-12.0))], **KW)
    (rep,), (l,) = tts.last_loudness, tts.last_limiter
    tts.infer_requests([_fmt(A, dict(hot, peak_dbfs=-12.0))], **KW)
    static, = tts.last_loudness
    print(f"0 LUFS under -12 dBFS: limiter {l}, gain {rep['gain_db']:.4f} dB against {static['gain_db']:.4f} dB with peak_dbfs")
    assert sr == 16000 and np.abs(w).max() <= np.float32(10.0 ** (-12.0 / 20)) and l["max_reduction_db"] > 0.0
    assert static["gain_db"] < rep["gain_db"] and abs(rep["gain_db"] - (0.0 - rep["measured_lufs"])) <= 1e-6


def test_last_limiter_is_filled_and_a_request_keeps_its_bytes_in_any_batch(tts, batch):
    (out_a, _, _), lim, _ = batch
    assert set(lim[0]) == {"max_reduction_db", "peak_dbfs_after"} and all(type(v) is float for v in lim[0].values())
    assert lim[0]["max_reduction_db"] >= 0.0 and lim[0]["peak_dbfs_after"] <= 20.0 * math.log10(float(O.AudioFormat.parse(LIMITED).ceiling))
    assert abs(lim[0]["peak_dbfs_after"] - 20.0 * math.log10(float(np.abs(out_a[1]).max()))) <= 1e-9       # the delivered samples' own peak
    (alone,), rep = tts.infer_requests([A], **KW), list(tts.last_limiter)
    back, rep_back = tts.infer_requests([C, B, A], **KW), list(tts.last_limiter)
    for got in (alone, back[2]):
        assert got[0] == out_a[0] and np.array_equal(got[1].view(np.uint8), out_a[1].view(np.uint8))
    assert rep == [lim[0]] and rep_back == [None, None, lim[0]]
    got = tts.infer_batch("alice.wav", ["hello world. and a second sentence", "ok. one more"], "en", audio_format="8000/pcm_f32le/-16lufs/-1limit",
                          num_beams=1, max_mel_tokens=24, cfm_noise="request", seed=5, interval_silence=40)
    assert len(tts.last_limiter) == 2 and all(isinstance(v, dict) for v in tts.last_limiter)
    assert all(sr == 8000 and np.abs(w).max() <= O.AudioFormat(limit_dbfs=-1.0).ceiling for sr, w in got)


def test_a_true_peak_target_is_met_as_the_meter_reads_the_delivered_samples(tts):
    fmt = dict(sample_rate=48000, encoding="pcm_f32le", peak_dbfs=-1.0, true_peak=True)
    (sr, w), = tts.infer_requests([_fmt(A, fmt)], **KW)
    (_, w_sample), = tts.infer_requests([_fmt(A, dict(fmt, true_peak=False))], **KW)
    got, sample = O.measure_true_peak(w[:, 0], DEV), 20.0 * math.log10(float(np.abs(w).max()))
    # the delivered samples are f32(y g): each within 2^-24 of y g, so their true peak is within (K + 3) 2^-24 sum |h| (the prototype's
    # largest phase) of g times the measured one -- the chain's forward bound plus the rounding of the scaled samples
    h = R.prototype_f32(1, 4)
    rel = (R.params(1, 4)[3] + 3) * U * max(float(np.abs(h[p::4]).sum()) for p in range(4))
    print(f"true-peak target -1 dBTP: delivered {got:.6f} dBTP (sample peak {sample:.4f} dBFS); the sample-peak form reads "
          f"{O.measure_true_peak(w_sample[:, 0], DEV):.4f} dBTP; tolerance {20 * math.log10(1 + rel):.2e} dB")
    tol = 20.0 * math.log10(1.0 + rel) + 1e-9
    assert sr == 48000 and abs(got - (-1.0)) <= tol and sample <= got + tol                   # (u[4n] is x[n] up to the chain's rounding)
    assert O.measure_true_peak(w_sample[:, 0], DEV) >= -1.0 - tol            # the sample-peak form is at least as hot in true peak
    assert tts.last_limiter == [None]


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


def test_a_stream_with_a_limiter_never_exceeds_its_ceiling_and_concatenates_to_the_one_shot_result(tts, alone):
    for req, ev in zip(STREAMS, alone):
        fmt = O.AudioFormat.parse(req["audio_format"])
        assert ev and ev[-1][2] and all(sr == fmt.sample_rate and p is not None and p.dtype == fmt.dtype for sr, p, _, _ in ev)
        floats = run_alone(tts, dict(req, audio_format="22050/pcm_f32le"))
        assert [(d, k) for _, _, d, k in floats] == [(d, k) for _, _, d, k in ev]
        whole = np.concatenate([p for _, p, _, _ in floats])
        one_shot, = O.convert([_dev(whole)], None, [[0]], fmt)
        cat = np.concatenate([p for _, p, _, _ in ev])
        L, M, _, _ = R.params(SRC, fmt.sample_rate)
        assert len(cat) == R.out_len(len(whole), L, M) and np.array_equal(cat, one_shot), req["audio_format"]
        if fmt.limit_dbfs is not None and fmt.encoding == "pcm_f32le":
            print(f"{req['audio_format']}: source peak {np.abs(whole).max():.4f}, gain {fmt.gain:.3f}, delivered peak {np.abs(cat).max():.6f}, "
                  f"ceiling {fmt.ceiling:.6f}; first pieces {[len(p) for _, p, _, _ in ev[:3]]}")
            assert np.abs(cat).max() <= fmt.ceiling                 # the +12 dB stream: never over the ceiling, an exact f32 compare


@pytest.mark.parametrize("slots, poll_steps", [(2, 8), (3, 3)])
def test_session_streams_are_bit_equal_to_the_request_alone(tts, alone, slots, poll_steps):
    with tts.stream_session(slots=slots, poll_steps=poll_steps, **SESSION) as sess:
        ids = [sess.submit(r) for r in STREAMS]
        with pytest.raises(ValueError, match="loudness_lufs"):
            sess.submit(dict(STREAMS[0], audio_format="8000/-16lufs/-1limit"))
        out = drain(sess)
    for i, sid in enumerate(ids):
        got, ref = out[sid], alone[i]
        assert [(sr, d, k) for sr, _, d, k in got] == [(sr, d, k) for sr, _, d, k in ref], i
        for (_, p, _, k), (_, p0, _, _) in zip(got, ref):
            assert p.dtype == p0.dtype and p.shape == p0.shape and np.array_equal(p, p0), (i, k)
