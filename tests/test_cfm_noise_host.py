"""The seeded flow-matching noise, host side (no GPU): the statistics of the generator as restated in tests/cfm_noise_ref.py, one pinned sample,
the additive C-ABI entry, and the `cfm_noise` option's argument handling in the pipeline.

Bounds of the statistics at N = 4096 frames x 80 channels = 327680 draws: four standard errors of the estimator under the null hypothesis
(mean: 1/sqrt(N); variance: sqrt(2/N); fourth moment: sqrt(96/N); a correlation: 1/sqrt(N)); the Kolmogorov-Smirnov bound is the 0.1 % critical
value 1.95/sqrt(N)."""
import math
import os

import numpy as np
import pytest
import torch

from tests.cfm_noise_ref import cfm_noise

FRAMES, CH = 4096, 80
N = FRAMES * CH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _z(seed, stream):
    if (seed, stream) not in _CACHE:
        z = cfm_noise(seed, stream, FRAMES, CH).astype(np.float64)
        z.setflags(write=False)
        _CACHE[(seed, stream)] = z
    return _CACHE[(seed, stream)]


def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


@pytest.mark.parametrize("seed", [7, 1234])
@pytest.mark.parametrize("stream", [0, 1])
def test_statistics_of_the_restated_generator(seed, stream):
    z = _z(seed, stream)
    mean, var = float(z.mean()), float(z.var())
    m4 = float((((z - mean) / math.sqrt(var)) ** 4).mean())
    zs = np.sort(z.ravel())
    cdf = torch.special.ndtr(torch.from_numpy(zs)).numpy()
    ks = float(max((np.arange(1, N + 1) / N - cdf).max(), (cdf - np.arange(0, N) / N).max()))
    lag_c, lag_f = _corr(z[:, :-1], z[:, 1:]), _corr(z[:-1], z[1:])
    cross = _corr(z, _z(seed, stream + 1))
    print(f"seed {seed} stream {stream}: mean {mean:+.4f} var-1 {var - 1:+.4f} m4-3 {m4 - 3:+.4f} KS {ks:.4f} lag-1 channels {lag_c:+.4f} "
          f"frames {lag_f:+.4f} stream s vs s+1 {cross:+.4f} max|z| {np.abs(z).max():.3f}")
    assert abs(mean) <= 4 / math.sqrt(N)
    assert abs(var - 1) <= 4 * math.sqrt(2 / N)
    assert abs(m4 - 3) <= 4 * math.sqrt(96 / N)
    assert ks <= 1.95 / math.sqrt(N)
    assert abs(lag_c) <= 4 / math.sqrt(N) and abs(lag_f) <= 4 / math.sqrt(N)
    assert abs(cross) <= 4 / math.sqrt(N)
    assert np.abs(z).max() <= 6.67                            # sqrt(-2 ln 2^-32) = 6.66


def test_pinned_sample():
    want = [[0.07671105, 0.961334, -1.3087327, -0.42896482], [0.94832146, 0.40955502, -0.0888237, 0.8197381]]
    got = cfm_noise(7, 2, 2, 4)
    assert got.dtype == np.float32 and got.shape == (2, 4)
    assert np.abs(got.astype(np.float64) - np.array(want)).max() <= 1e-6
    # the counter is frame * C + channel, relative to the first target frame; temperature scales; the chunk is part of the key
    assert np.array_equal(cfm_noise(7, 2, 1, 4, first_frame=1)[0], got[1])
    assert np.abs(cfm_noise(7, 2, 2, 4, temperature=0.5) - 0.5 * got).max() <= 1e-7
    assert not np.array_equal(cfm_noise(7, 2, 2, 4, chunk=1), got)
    assert np.array_equal(cfm_noise(2 ** 63 + 5, 0, 3, 6), cfm_noise(2 ** 63 + 5, 0, 3, 6))


def test_header_documents_the_additive_entry_and_keeps_the_abi_version():
    with open(os.path.join(ROOT, "include", "indextts_hip.h")) as f:
        h = f.read()
    assert "#define ITTS_ABI_VERSION 13" in h
    assert "v13, additive: seeded flow-matching noise" in h
    assert "int itts_s2mel_noise_forward(" in h
    assert "0x43464D4E4F495345" in h and "flow_matching.py:31-55" in h


def test_lib_declares_the_entry():
    from indextts_amd import _lib
    restype, argtypes = _lib.SIGNATURES["itts_s2mel_noise_forward"]
    assert len(argtypes) == 11


def _cpu_pipeline():
    from tests.test_pipeline_cpu import make
    return make()[0]


def test_unknown_cfm_noise_value_raises():
    tts = _cpu_pipeline()
    with pytest.raises(ValueError, match="cfm_noise"):
        tts.infer_batch("spk.wav", ["hello there"], "en", num_beams=1, cfm_noise="per-row")
    with pytest.raises(ValueError, match="cfm_noise"):
        tts.infer_requests([dict(spk_audio_prompt="spk.wav", text="hello there", lang="en")], num_beams=1, cfm_noise="slot")
    with pytest.raises(ValueError, match="cfm_noise"):
        next(tts.infer_stream("spk.wav", ["hello there"], "en", cfm_noise=""))
    assert tts.gpt.calls == []                                  # refused before any work


def test_option_never_reaches_the_gpt_and_the_default_is_the_old_path():
    tts = _cpu_pipeline()
    a = tts.infer_batch("spk.wav", ["hello there. again"], "en", num_beams=1)
    b = tts.infer_batch("spk.wav", ["hello there. again"], "en", num_beams=1, cfm_noise="global")
    assert np.array_equal(a[0][1], b[0][1])
    assert all("cfm_noise" not in kw for _, kw in tts.gpt.calls) and tts.gpt.calls[0][1].keys() == tts.gpt.calls[1][1].keys()


def test_keyed_noise_and_request_settings_need_the_engine_stages():
    tts = _cpu_pipeline()                                      # codes -> mel on the frontend's (here: stub) PyTorch path
    req = dict(spk_audio_prompt="spk.wav", text="hello there", lang="en")
    with pytest.raises(ValueError, match="engine"):
        tts.infer_batch("spk.wav", ["hello there"], "en", num_beams=1, cfm_noise="request")
    with pytest.raises(ValueError, match="engine"):
        tts.infer_requests([req], num_beams=1, cfm_noise="request")
    for key, val in (("diffusion_steps", 10), ("inference_cfg_rate", 0.5), ("cfm_temperature", 0.9)):
        with pytest.raises(ValueError, match="request 1.*engine"):
            tts.infer_requests([req, dict(req, **{key: val})], num_beams=1)
        with pytest.raises(ValueError, match="engine"):
            tts.infer_requests([req], num_beams=1, **{key: val})
    with pytest.raises(ValueError, match=r"request 0: unknown keys \['cfm_steps'\]"):
        tts.infer_requests([dict(req, cfm_steps=3)], num_beams=1)


def test_request_setting_ranges_name_the_request():
    tts = _cpu_pipeline()
    tts.s2mel = tts.semantic_codec = object()                  # "engine stages present": the range checks run before any of them is used
    req = dict(spk_audio_prompt="spk.wav", text="hello there", lang="en")
    for key, val in (("diffusion_steps", 0), ("diffusion_steps", 2.5), ("inference_cfg_rate", -0.1), ("cfm_temperature", -1.0),
                     ("cfm_temperature", float("nan"))):
        with pytest.raises(ValueError, match=f"request 1: `{key}`"):
            tts.infer_requests([req, dict(req, **{key: val})], num_beams=1)


def test_batcher_keeps_the_option_call_wide_and_the_settings_per_request():
    from indextts_amd.serving import DynamicBatcher

    class Rec:
        def __init__(self):
            self.calls = []

        def infer_requests(self, reqs, **kw):
            self.calls.append((reqs, kw))
            return [(22050, np.zeros((1, 1), np.int16))] * len(reqs)

    rec = Rec()
    b = DynamicBatcher(rec, max_batch=2, max_wait_ms=2000.0, mixed=True)
    try:
        f = [b.submit("a.wav", "one", "en", num_beams=1, cfm_noise="request", seed=3, diffusion_steps=10),
             b.submit("b.wav", "two", "en", num_beams=1, cfm_noise="request", seed=4, cfm_temperature=0.8)]
        for x in f:
            x.result(timeout=30)
    finally:
        b.close()
    assert len(rec.calls) == 1                                  # one batch: the per-request settings do not split the group
    reqs, kw = rec.calls[0]
    assert kw == dict(num_beams=1, cfm_noise="request")
    assert reqs[0]["diffusion_steps"] == 10 and reqs[0]["seed"] == 3 and reqs[1]["cfm_temperature"] == 0.8 and "diffusion_steps" not in reqs[1]
