"""CPU tests of per-request settings under beam search: the per-group sampling table's declaration, host image and validation
(`gpt.group_sampling_entries`, `itts_gpt_set_group_sampling`), the table and caps `IndexTTS2.infer_requests(beam_settings="own")` hands to the
GPT (a recording stub), the unchanged refusal of the default `beam_settings="shared"`, and the serving shell forwarding the option."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from indextts_amd import _lib, gpt
from tests.pipeline_stubs import StubFrontend

DEFAULTS = dict(do_sample=1, top_k=30, top_p=0.8, temperature=0.8, repetition_penalty=10.0, typical_mass=0.0, seed=5, length_penalty=0.0)


def test_entry_is_declared_exported_and_laid_out_as_the_header_says():
    hdr = open(os.path.join(_lib.HERE, "..", "include", "indextts_hip.h")).read()
    assert "int itts_gpt_set_group_sampling(itts_gpt* h, const itts_group_sampling* table, int n_groups);" in hdr
    assert "v13, additive: per-group sampling table" in hdr and "#define ITTS_ABI_VERSION 13" in hdr
    comment = hdr[hdr.index("per-group sampling table"):hdr.index("} itts_group_sampling;")]
    assert "infer_v2_5.py:732-740" in comment and "backends/trt/serving/triton_server.py:96-305" in comment       # what it replaces
    assert "itts_gpt_set_group_sampling" in _lib.SIGNATURES and hasattr(_lib.lib(), "itts_gpt_set_group_sampling")
    # int32 x 3 | f32 x 5 | int32 stream | 4 pad bytes | uint64 seed
    G = _lib.GroupSampling
    assert C.sizeof(G) == 48
    assert [getattr(G, f).offset for f in ("do_sample", "top_k", "min_tokens_to_keep", "top_p", "temperature", "repetition_penalty", "typical_mass",
                                           "length_penalty", "stream", "seed")] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    struct = comment[comment.index("typedef struct"):]
    assert [w for w in ("do_sample", "top_k", "min_tokens_to_keep", "top_p", "temperature", "repetition_penalty", "typical_mass", "length_penalty",
                        "stream", "seed") if w in struct] == [f[0] for f in G._fields_]
    assert _lib.lib().itts_gpt_set_group_sampling(None, None, 0) == _lib.ERR_ARG       # host-only check: no GPU needed


def test_group_sampling_entries_defaults_and_host_image():
    e = gpt.group_sampling_entries([{}, dict(temperature=1.5, stream=0, seed=9, do_sample=False, length_penalty=1.0)], 2, DEFAULTS)
    assert (e[0].do_sample, e[0].top_k, e[0].stream, e[0].seed, e[0].min_tokens_to_keep) == (1, 30, 0, 5, 2)     # beams keep eos + 1
    assert abs(e[0].top_p - 0.8) < 1e-7 and abs(e[0].repetition_penalty - 10.0) < 1e-7 and e[0].length_penalty == 0.0
    assert (e[1].do_sample, e[1].stream, e[1].seed, e[1].length_penalty) == (0, 0, 9, 1.0) and abs(e[1].temperature - 1.5) < 1e-7
    assert gpt.group_sampling_entries([{}, {}], 2, DEFAULTS)[1].stream == 1                     # default stream: the slot index
    assert gpt.group_sampling_entries([{}], 1, DEFAULTS, slots=[3])[0].stream == 3              # ... of the slot an admission fills
    assert gpt.group_sampling_entries([{}], 1, dict(DEFAULTS, min_tokens_to_keep=1))[0].min_tokens_to_keep == 1
    img = gpt._group_sampling_bytes(e)
    assert img.shape == (2, 48) and img.dtype == torch.uint8
    back = np.frombuffer(img.numpy().tobytes(), dtype=np.dtype([("i", "<i4", 3), ("f", "<f4", 5), ("stream", "<i4"), ("pad", "<i4"), ("seed", "<u8")]))
    assert back["i"].tolist() == [[1, 30, 2], [0, 30, 2]] and back["seed"].tolist() == [5, 9] and back["stream"].tolist() == [0, 0]
    assert back["f"][:, 4].tolist() == [0.0, 1.0]                                               # length_penalty is the fifth float


@pytest.mark.parametrize("bad, exc", [
    (dict(top_k=0), ValueError), (dict(top_k=65), ValueError), (dict(typical_mass=1.0), ValueError), (dict(typical_mass=-0.1), ValueError),
    (dict(temperature=0.0), ValueError), (dict(repetition_penalty=0.0), ValueError), (dict(repetition_penalty=-2.0), ValueError),
    (dict(min_tokens_to_keep=3), ValueError), (dict(nucleus=0.5), ValueError), (dict(stream=2 ** 31), ValueError), ("beam", TypeError)])
def test_group_sampling_validation_raises_for_bad_entries(bad, exc):
    with pytest.raises(exc):
        gpt.group_sampling_entries([{}, bad], 2, DEFAULTS)


def test_group_sampling_needs_one_entry_per_utterance_and_beam_search_ignores_top_k():
    with pytest.raises(ValueError, match="one entry per utterance"):
        gpt.group_sampling_entries([{}], 2, DEFAULTS)
    assert gpt.group_sampling_entries([dict(do_sample=False, top_k=0)], 1, DEFAULTS)[0].top_k == 0   # as the scalar path: top_k binds only sampling
    with pytest.raises(ValueError, match="unknown keys"):                                            # length_penalty is no key of a num_beams = 1 entry
        gpt.row_sampling_entries([dict(length_penalty=1.0)], 1, DEFAULTS)


# ---- infer_requests over a recording GPT stub ------------------------------------------------------------------------------------------------
class _Recorded(Exception):
    pass


class _StubGPT:
    """what `infer_requests` touches up to the generate call, which is recorded and ends the run"""
    n_text_pos = 600

    def __init__(self):
        self.calls, self._next = [], 1000

    def conds_latent(self, style, emovec):
        return torch.zeros(1, 3, 8), None

    def _seed(self, seed, do_sample, uniforms):
        if seed is not None:
            return int(seed)
        self._next += 1
        return self._next

    def inference_speech(self, *a, **kw):
        self.calls.append(("inference_speech", kw))
        raise _Recorded

    def inference_speech_inflight_beams(self, *a, **kw):
        self.calls.append(("inference_speech_inflight_beams", kw))
        raise _Recorded


def _pipeline():
    from indextts_amd.infer_v2_5 import IndexTTS2
    from indextts_amd.serving import SpeakerCache
    t = object.__new__(IndexTTS2)
    t.frontend, t.gpt, t.device = StubFrontend(8), _StubGPT(), "cpu"
    t.speaker_cache = SpeakerCache(lambda a: t.frontend.speaker_bundle(a))
    t.emotion_cache = SpeakerCache(lambda a: t.frontend.emo_cond(a))
    return t


REQS = [dict(spk_audio_prompt="a.wav", text="one. two", lang="en", temperature=0.7, top_p=0.9, seed=11, length_penalty=1.0),
        dict(spk_audio_prompt="b.wav", text="three", lang="en", top_k=8, max_mel_tokens=9, typical_sampling=True, typical_mass=0.5),
        dict(spk_audio_prompt="a.wav", text="four", lang="en", repetition_penalty=2.0, seed=13)]


def test_infer_requests_own_builds_the_group_table_and_caps():
    t = _pipeline()
    with pytest.raises(_Recorded):
        t.infer_requests(REQS, beam_settings="own", max_mel_tokens=24, length_penalty=0.5)
    (name, kw), = t.gpt.calls
    assert name == "inference_speech" and kw["num_beams"] == 3 and kw["do_sample"] is True
    assert kw["row_max_new"] == [24, 24, 9, 24] and kw["max_generate_length"] == 24 and "beam_settings" not in kw
    tab = kw["group_sampling"]
    assert len(tab) == 4 and all(e["do_sample"] is True for e in tab)
    assert [e["stream"] for e in tab] == [0, 1, 0, 0]                          # the segment's index in its request
    assert [e["seed"] for e in tab] == [11, 11, 1001, 13]                      # one per request; the request without one draws it
    assert [e["length_penalty"] for e in tab] == [1.0, 1.0, 0.5, 0.5]          # a request key in this mode, else the call's
    assert [e["temperature"] for e in tab] == [0.7, 0.7, 0.8, 0.8] and [e["top_p"] for e in tab] == [0.9, 0.9, 0.8, 0.8]
    assert [e["top_k"] for e in tab] == [30, 30, 8, 30] and [e["repetition_penalty"] for e in tab] == [10.0, 10.0, 10.0, 2.0]
    assert [e["typical_mass"] for e in tab] == [0.0, 0.0, 0.5, 0.0]
    gpt.group_sampling_entries(tab, 4, DEFAULTS)                               # and the engine's host check accepts every entry
    # more utterances than beam slots: the session path gets the same table
    t2 = _pipeline()
    with pytest.raises(_Recorded):
        t2.infer_requests(REQS, beam_settings="own", max_mel_tokens=24, inflight_beam_slots=2)
    (name2, kw2), = t2.gpt.calls
    assert name2 == "inference_speech_inflight_beams" and kw2["slots"] == 2 and kw2["row_max_new"] == [24, 24, 9, 24]
    assert [e["stream"] for e in kw2["group_sampling"]] == [0, 1, 0, 0]


def test_infer_requests_shared_keeps_its_refusal_and_names_the_option():
    t = _pipeline()
    with pytest.raises(ValueError, match="share") as ei:
        t.infer_requests(REQS[1:], max_mel_tokens=24)
    assert "beam_settings" in str(ei.value) and not t.gpt.calls
    with pytest.raises(ValueError, match="unknown keys"):                      # length_penalty is a request key with beam_settings="own" only
        t.infer_requests(REQS[:1], max_mel_tokens=24)
    with pytest.raises(ValueError, match="unknown keys"):
        t.infer_requests(REQS[:1], num_beams=1, beam_settings="own", max_mel_tokens=24)
    with pytest.raises(ValueError, match="beam_settings"):
        t.infer_requests(REQS[1:], beam_settings="each")
    # requests that agree still run as today: one scalar beam call, no table
    same = [dict(r, top_p=0.6) for r in (dict(spk_audio_prompt="a.wav", text="x", lang="en"), dict(spk_audio_prompt="b.wav", text="y", lang="en"))]
    with pytest.raises(_Recorded):
        t.infer_requests(same, max_mel_tokens=24)
    kw = t.gpt.calls[0][1]
    assert "group_sampling" not in kw and "row_max_new" not in kw and kw["top_p"] == 0.6 and kw["max_generate_length"] == 24


# ---- the serving shell -----------------------------------------------------------------------------------------------------------------------
class _FakeTTS:
    def __init__(self):
        self.request_calls = []

    def infer_requests(self, requests, **defaults):
        self.request_calls.append(([dict(r) for r in requests], dict(defaults)))
        return [(22050, np.full((len(r["text"]), 1), len(r["spk_audio_prompt"]), dtype=np.int16)) for r in requests]


def test_dynamic_batcher_mixed_forwards_beam_settings_and_merges_the_settings():
    from indextts_amd.serving import DynamicBatcher
    tts = _FakeTTS()
    b = DynamicBatcher(tts, max_batch=4, max_wait_ms=2000, mixed=True)
    voices = [b"A", b"BB"]
    futs = [b.submit(voices[i % 2], "t" * (i + 1), "en", beam_settings="own", top_p=0.8 if i < 2 else 0.6, seed=i) for i in range(4)]
    outs = [f.result(timeout=10) for f in futs]
    b.close()
    assert b.batches == [4] and len(tts.request_calls) == 1                    # 3-beam requests with their own settings share ONE batch
    reqs, defaults = tts.request_calls[0]
    assert defaults == {"beam_settings": "own"}
    assert [r["top_p"] for r in reqs] == [0.8, 0.8, 0.6, 0.6] and [r["seed"] for r in reqs] == [0, 1, 2, 3]
    for i, (sr, w) in enumerate(outs):
        assert sr == 22050 and w.shape[0] == i + 1 and int(w[0, 0]) == len(voices[i % 2])


def test_synthesize_tasks_mixed_forwards_beam_settings(tmp_path):
    from indextts_amd.serving import synthesize_tasks
    tts = _FakeTTS()
    tasks = [dict(voice_path=f"v{i % 2}.wav", text="x" * (i + 2), output_path=tmp_path / f"{i}.wav", line_number=i + 1) for i in range(3)]
    synthesize_tasks(tts, tasks, lang="en", max_batch=4, mixed=True, beam_settings="own")
    assert [len(c[0]) for c in tts.request_calls] == [3] and tts.request_calls[0][1] == {"beam_settings": "own"}


# ---- the builders every generate call and session shares (indextts_amd/gpt.py) ----
GP_FIELDS = ("do_sample", "num_beams", "top_k", "min_tokens_to_keep", "max_new_tokens", "pos_offset", "top_p", "temperature", "repetition_penalty",
             "length_penalty", "typical_mass", "reserved", "seed")


def _gp_fields(gp):
    return {f: getattr(gp, f) for f in GP_FIELDS}


@pytest.mark.parametrize("num_beams,keep", [(1, 1), (3, 2)])
@pytest.mark.parametrize("kv_cache,pos_offset", [(True, 2), (False, 1)])
def test_gen_params_builder_field_by_field(num_beams, keep, kv_cache, pos_offset):
    gp = gpt._gen_params(kv_cache, 40, 77, do_sample=True, num_beams=num_beams, top_p=0.5, top_k=30, temperature=2.0, repetition_penalty=None,
                         length_penalty=0.25, typical_mass=0.75)
    assert _gp_fields(gp) == dict(do_sample=1, num_beams=num_beams, top_k=30, min_tokens_to_keep=keep, max_new_tokens=40, pos_offset=pos_offset,
                                  top_p=0.5, temperature=2.0, repetition_penalty=1.0, length_penalty=0.25, typical_mass=0.75, reserved=0, seed=77)
    # the defaults are `generate`'s; top_k=None is "no top-k"
    assert _gp_fields(gpt._gen_params(kv_cache, 7, 0, num_beams=num_beams, top_k=None)) == dict(
        do_sample=0, num_beams=num_beams, top_k=0, min_tokens_to_keep=keep, max_new_tokens=7, pos_offset=pos_offset, top_p=1.0, temperature=1.0,
        repetition_penalty=1.0, length_penalty=1.0, typical_mass=0.0, reserved=0, seed=0)


@pytest.mark.parametrize("nb", [1, 3])
def test_prefix_builder_appends_the_start_row_and_repeats_per_beam(nb):
    m = object.__new__(gpt.UnifiedVoice)
    m.device, m.start_mel_token = torch.device("cpu"), 2
    D, s = 4, 5
    m._emb = {"mel_embedding.weight": torch.arange(3 * D, dtype=torch.float32).view(3, D), "mel_pos_embedding.emb.weight": torch.full((6, D), 0.5)}
    emb = torch.randn(2, s, D, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    mask = torch.ones(2, s + 1, dtype=torch.long)
    mask[0, :3], mask[1, :1] = 0, 0                                # rows left-padded by 3 and by 1
    x, pad, S = m._prefix(emb, mask, nb)
    assert S == s + 1 and x.shape == (2 * nb, S, D) and x.dtype == torch.float32 and x.is_contiguous()
    assert pad.dtype == torch.int32 and pad.tolist() == [3] * nb + [1] * nb          # per row, repeated per beam
    start = m._emb["mel_embedding.weight"][2] + 0.5
    for b in range(2):
        for j in range(nb):                                        # beams adjacent: rows b * nb .. b * nb + nb - 1 carry utterance b
            assert torch.equal(x[b * nb + j, :s], emb[b].float()) and torch.equal(x[b * nb + j, s], start)
