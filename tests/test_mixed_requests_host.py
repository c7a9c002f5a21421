"""CPU tests of the mixed-request path: the per-slot sampling table's host image and validation (`gpt.row_sampling_entries`), the engine
entry's declaration, and the serving shell's mixed mode (`DynamicBatcher(mixed=True)`, `synthesize_tasks(mixed=True)`) over a recording
fake pipeline."""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

from indextts_amd import _lib, gpt

DEFAULTS = dict(do_sample=1, top_k=30, top_p=0.8, temperature=0.8, repetition_penalty=10.0, typical_mass=0.0, seed=5)


def test_entry_is_declared_exported_and_laid_out_as_the_header_says():
    hdr = open(os.path.join(_lib.HERE, "..", "include", "indextts_hip.h")).read()
    assert "int itts_gpt_set_row_sampling(itts_gpt* h, const itts_row_sampling* table, int n);" in hdr
    assert "v13, additive: per-slot sampling table" in hdr and "#define ITTS_ABI_VERSION 13" in hdr
    assert "backends/trt/serving/triton_server.py:96-305" in hdr[hdr.index("per-slot sampling table"):hdr.index("} itts_row_sampling;")]
    assert "itts_gpt_set_row_sampling" in _lib.SIGNATURES and hasattr(_lib.lib(), "itts_gpt_set_row_sampling")
    assert C.sizeof(_lib.RowSampling) == 40 and _lib.RowSampling.seed.offset == 32 and _lib.RowSampling.stream.offset == 28
    assert _lib.lib().itts_gpt_set_row_sampling(None, None, 0) == _lib.ERR_ARG       # host-only check: no GPU needed


def test_row_sampling_entries_defaults_and_host_image():
    e = gpt.row_sampling_entries([{}, dict(temperature=1.5, stream=0, seed=9, do_sample=False)], 2, DEFAULTS)
    assert (e[0].do_sample, e[0].top_k, e[0].stream, e[0].seed, e[0].min_tokens_to_keep) == (1, 30, 0, 5, 1)
    assert abs(e[0].top_p - 0.8) < 1e-7 and abs(e[0].repetition_penalty - 10.0) < 1e-7
    assert (e[1].do_sample, e[1].stream, e[1].seed) == (0, 0, 9) and abs(e[1].temperature - 1.5) < 1e-7
    assert gpt.row_sampling_entries([{}, {}], 2, DEFAULTS)[1].stream == 1                       # default stream: the slot index
    assert gpt.row_sampling_entries([{}], 1, DEFAULTS, slots=[3])[0].stream == 3                # ... of the slot an admission fills
    img = gpt._row_sampling_bytes(e)
    assert img.shape == (2, 40) and img.dtype == torch.uint8
    back = np.frombuffer(img.numpy().tobytes(), dtype=np.dtype([("i", "<i4", 3), ("f", "<f4", 4), ("stream", "<i4"), ("seed", "<u8")]))
    assert back["i"].tolist() == [[1, 30, 1], [0, 30, 1]] and back["seed"].tolist() == [5, 9] and back["stream"].tolist() == [0, 0]


@pytest.mark.parametrize("bad, exc", [
    (dict(top_k=0), ValueError), (dict(top_k=65), ValueError), (dict(typical_mass=1.0), ValueError), (dict(typical_mass=-0.1), ValueError),
    (dict(temperature=0.0), ValueError), (dict(repetition_penalty=0.0), ValueError), (dict(repetition_penalty=-2.0), ValueError),
    (dict(min_tokens_to_keep=3), ValueError), (dict(nucleus=0.5), ValueError), (dict(stream=2 ** 31), ValueError), ("greedy", TypeError)])
def test_row_sampling_validation_raises_for_bad_entries(bad, exc):
    with pytest.raises(exc):
        gpt.row_sampling_entries([{}, bad], 2, DEFAULTS)


def test_row_sampling_needs_one_entry_per_row_and_greedy_ignores_top_k():
    with pytest.raises(ValueError, match="one entry per row"):
        gpt.row_sampling_entries([{}], 2, DEFAULTS)
    assert gpt.row_sampling_entries([dict(do_sample=False, top_k=0)], 1, DEFAULTS)[0].top_k == 0     # as the scalar path: top_k binds only sampling


class _FakeTTS:
    """records every pipeline call; a result's length is the text's, its value the voice's length"""

    def __init__(self):
        self.batch_calls, self.request_calls = [], []

    def infer_batch(self, spk, texts, lang, emo_audio_prompt=None, emo_alpha=1.0, **gen):
        self.batch_calls.append((spk, list(texts), dict(gen)))
        return [(22050, np.full((len(t), 1), len(spk), dtype=np.int16)) for t in texts]

    def infer_requests(self, requests, **defaults):
        self.request_calls.append(([dict(r) for r in requests], dict(defaults)))
        return [(22050, np.full((len(r["text"]), 1), len(r["spk_audio_prompt"]), dtype=np.int16)) for r in requests]


def test_dynamic_batcher_mixed_merges_voices_and_sampling_settings():
    from indextts_amd.serving import DynamicBatcher
    tts = _FakeTTS()
    b = DynamicBatcher(tts, max_batch=6, max_wait_ms=2000, mixed=True)
    voices = [b"A", b"BB", b"CCC"]
    futs = [b.submit(voices[i % 3], "t" * (i + 1), "en" if i % 2 else "zh", num_beams=1, top_p=0.8 if i < 3 else 0.6) for i in range(6)]
    outs = [f.result(timeout=10) for f in futs]
    assert b.batches == [6] and len(tts.request_calls) == 1 and not tts.batch_calls
    reqs, defaults = tts.request_calls[0]
    assert defaults == {"num_beams": 1}
    assert [r["top_p"] for r in reqs] == [0.8] * 3 + [0.6] * 3 and [r["spk_audio_prompt"] for r in reqs] == [voices[i % 3] for i in range(6)]
    for i, (sr, w) in enumerate(outs):                           # each future gets its own result
        assert sr == 22050 and w.shape[0] == i + 1 and int(w[0, 0]) == len(voices[i % 3])
    # beams: the sampling settings are call-wide, so they group; voices still mix
    f1 = [b.submit(voices[i], "beam", "en", top_p=0.8) for i in range(3)] + [b.submit(b"A", "other", "en", top_p=0.5)]
    [f.result(timeout=10) for f in f1]
    b.close()
    assert sorted(b.batches[1:]) == [1, 3]
    three = [c for c in tts.request_calls[1:] if len(c[0]) == 3][0]
    assert {r["spk_audio_prompt"] for r in three[0]} == set(voices) and all(r["top_p"] == 0.8 for r in three[0])


def test_dynamic_batcher_default_is_unchanged():
    from indextts_amd.serving import DynamicBatcher
    tts = _FakeTTS()
    b = DynamicBatcher(tts, max_batch=6, max_wait_ms=50)
    futs = [b.submit([b"A", b"BB", b"CCC"][i % 3], f"t{i}", "en", num_beams=1, top_p=0.8 if i < 3 else 0.6) for i in range(6)]
    [f.result(timeout=10) for f in futs]
    b.close()
    assert b.batches == [1] * 6 and not tts.request_calls and len(tts.batch_calls) == 6          # six groups: voice x top_p


def test_synthesize_tasks_mixed_writes_every_file_from_cross_voice_batches(tmp_path):
    from indextts_amd.serving import synthesize_tasks
    tts = _FakeTTS()
    tasks = [dict(voice_path=f"v{i % 3}.wav", text="x" * (i + 2), output_path=tmp_path / "out" / f"{i}.wav", line_number=i + 1) for i in range(5)]
    tasks[1]["emotion_kwargs"] = {"emo_alpha": 0.5, "emo_audio_prompt": "sad.wav"}
    paths = synthesize_tasks(tts, tasks, lang="en", max_batch=4, mixed=True, num_beams=1)
    assert [len(c[0]) for c in tts.request_calls] == [4, 1] and not tts.batch_calls
    first = tts.request_calls[0][0]
    assert len({r["spk_audio_prompt"] for r in first}) == 3 and first[1]["emo_alpha"] == 0.5 and first[0]["lang"] == "en"
    assert tts.request_calls[0][1] == {"num_beams": 1}
    assert paths == [str(t["output_path"]) for t in tasks]
    for i, p in enumerate(paths):
        with wave.open(p, "rb") as w:
            assert (w.getframerate(), w.getnframes()) == (22050, i + 2)
    # unchanged default: one infer_batch call per voice
    tts2 = _FakeTTS()
    synthesize_tasks(tts2, tasks[:1] + tasks[2:], lang="en", max_batch=4)
    assert [c[0] for c in tts2.batch_calls] == ["v0.wav", "v2.wav", "v1.wav"] and not tts2.request_calls
