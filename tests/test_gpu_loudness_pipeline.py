"""`audio_format=` with `loudness_lufs` through the pipeline entries on the real HIP engines (the tiny models of tests/test_gpu_output_pipeline.py):
a request is delivered at its target as tests/loudness_ref.py reads the decoded samples, an unformatted request in the same batch is untouched,
`last_loudness` is the reference's measurement of the un-normalised conversion, the bytes are those of the request alone in any batch order, and
a ceiling that binds is met to one quantisation step."""
import math

import numpy as np
import pytest
import torch

from indextts_amd import output as O
from tests import loudness_ref as LR
from tests.test_gpu_cfm_noise_pipeline import VoiceFrontend
from tests.test_gpu_pipeline import _s2_engines, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SRC = 22050
KW = dict(num_beams=1, max_mel_tokens=24, cfm_noise="request", interval_silence=40)
TARGET = -30.0

A = dict(spk_audio_prompt="alice.wav", text="hello world. and a second sentence", lang="en", seed=11,
         audio_format=dict(sample_rate=48000, encoding="pcm_f32le", loudness_lufs=TARGET))
B = dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=12, temperature=1.1, top_k=12,
         audio_format=dict(sample_rate=8000, encoding="pcm_s16le", loudness_lufs=TARGET))
C = dict(spk_audio_prompt="carol.wav", text="a much longer second sentence here. ok", lang="en", seed=13)


@pytest.fixture(scope="module")
def tts():
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    t.semantic_codec, t.s2mel = _s2_engines("fp32")[:2]
    return t


@pytest.fixture(scope="module")
def batch(tts):
    out = tts.infer_requests([A, B, C], **KW)
    return out, list(tts.last_loudness)


def _plain(req):
    return {k: v for k, v in req.items() if k != "audio_format"}


def _resampled(tts, req, rate):
    """the request's un-normalised f32 signal at `rate`, as `convert` measures it: its 22050 Hz float rows through the device resampler"""
    (sr, w), = tts.infer_requests([dict(_plain(req), audio_format="22050/pcm_f32le")], **KW)
    assert sr == SRC and w.dtype == np.float32
    x = torch.from_numpy(np.ascontiguousarray(w[:, 0])).to(DEV)
    L, M, _, _ = O.resample_params(SRC, rate)
    n_out = O.resampled_length(x.numel(), L, M)
    return O.resample_seq(x, [(0, x.numel(), 0, 0, 0, n_out, 1)], SRC, rate, n_out)[:n_out].cpu().numpy()


def test_requests_are_delivered_at_their_target_and_the_unformatted_one_is_untouched(tts, batch):
    (out_a, out_b, out_c), loud = batch
    (sr_c, w_c), = tts.infer_requests([C], **KW)
    assert out_c[0] == sr_c == SRC and out_c[1].dtype == np.int16 and np.array_equal(out_c[1], w_c)      # C: the bytes of the call without A and B
    assert loud[2] is None and isinstance(loud[0], dict) and isinstance(loud[1], dict)
    sr, w = out_a
    assert sr == 48000 and w.dtype == np.float32 and w.ndim == 2 and np.abs(w).max() < 1.0               # nothing at full scale
    got = LR.loudness(w[:, 0], 48000)
    print(f"A (48000/pcm_f32le): {got:.7f} LUFS, report {loud[0]}")
    assert abs(got - TARGET) <= 1e-4
    sr, w = out_b
    assert sr == 8000 and w.dtype == np.int16 and np.abs(w.astype(np.int32)).max() < 32767
    got = LR.loudness(w[:, 0].astype(np.float64) / 32767.0, 8000)
    print(f"B (8000/pcm_s16le): {got:.7f} LUFS, report {loud[1]}")
    assert abs(got - TARGET) <= 1e-3


def test_last_loudness_is_the_reference_on_the_unnormalised_conversion(tts, batch):
    _, loud = batch
    for req, rep in ((A, loud[0]), (B, loud[1])):
        rate = req["audio_format"]["sample_rate"]
        x = _resampled(tts, req, rate)
        m = LR.measure(x, rate)
        assert set(rep) == {"measured_lufs", "gain_db", "peak_dbfs_after"} and all(type(v) is float for v in rep.values())
        print(f"{rate} Hz: measured {rep['measured_lufs']:.9f}, reference {m['lufs']:.9f} ({m['kept']} of {m['n_blocks']} blocks)")
        assert math.isfinite(m["lufs"]) and abs(rep["measured_lufs"] - m["lufs"]) <= 1e-6
        g = LR.gain(rep["measured_lufs"], TARGET)
        assert abs(rep["gain_db"] - 20.0 * math.log10(float(g))) <= 1e-9
        assert abs(rep["peak_dbfs_after"] - 20.0 * math.log10(float(np.float32(np.abs(x).max()) * g))) <= 1e-9


def test_a_request_gets_the_same_bytes_alone_in_a_batch_and_in_the_reversed_batch(tts, batch):
    (out_a, out_b, _), loud = batch
    (alone_a,), rep_a = tts.infer_requests([A], **KW), list(tts.last_loudness)
    back, rep_back = tts.infer_requests([C, B, A], **KW), list(tts.last_loudness)
    for got in (alone_a, back[2]):
        assert got[0] == out_a[0] and np.array_equal(got[1].view(np.uint8), out_a[1].view(np.uint8))
    assert back[1][0] == out_b[0] and np.array_equal(back[1][1], out_b[1])
    assert rep_a == [loud[0]] and rep_back == [None, loud[1], loud[0]]           # the same f64 measurement, bit for bit


def test_a_ceiling_that_binds_is_met_to_one_step_and_the_loudness_stays_below_the_target(tts):
    # no signal reads 0 LUFS with its peak 12 dB under full scale: the ceiling binds
    fmt = dict(sample_rate=16000, encoding="pcm_s16le", loudness_lufs=0.0, peak_dbfs=-12.0)
    (sr, w), = tts.infer_requests([dict(_plain(A), audio_format=fmt)], **KW)
    rep, = tts.last_loudness
    assert sr == 16000 and w.dtype == np.int16
    peak = float(np.abs(w.astype(np.int32)).max()) / 32767.0
    got = LR.loudness(w[:, 0].astype(np.float64) / 32767.0, 16000)
    print(f"ceiling -12 dBFS: delivered peak {20 * math.log10(peak):.5f} dBFS, {got:.4f} LUFS, report {rep}")
    assert abs(peak - 10.0 ** (-12.0 / 20.0)) <= 1.0 / 32767.0
    assert got < 0.0 - 1.0 and rep["gain_db"] < 0.0 - rep["measured_lufs"] and abs(rep["peak_dbfs_after"] - (-12.0)) <= 1e-5
    # the same target without a ceiling it can reach: the ceiling does not bind and the target is met
    fmt = dict(sample_rate=16000, encoding="pcm_f32le", loudness_lufs=TARGET, peak_dbfs=-1.0)
    (sr, w), = tts.infer_requests([dict(_plain(A), audio_format=fmt)], **KW)
    assert abs(LR.loudness(w[:, 0], 16000) - TARGET) <= 1e-4 and np.abs(w).max() < 10.0 ** (-1.0 / 20.0)


def test_infer_batch_takes_the_target(tts):
    texts = ["hello world. and a second sentence", "ok. one more sentence for the batch"]
    kw = dict(num_beams=1, max_mel_tokens=24, cfm_noise="request", seed=5, interval_silence=40)
    got = tts.infer_batch("alice.wav", texts, "en", audio_format="8000/pcm_f32le/-30lufs", **kw)
    assert len(tts.last_loudness) == 2
    for (sr, w), rep in zip(got, tts.last_loudness):
        assert sr == 8000 and w.dtype == np.float32 and math.isfinite(rep["measured_lufs"])
        assert abs(LR.loudness(w[:, 0], 8000) - TARGET) <= 1e-4
    tts.infer_batch("alice.wav", texts, "en", audio_format="8000/pcm_f32le", **kw)
    assert tts.last_loudness == [None, None]
