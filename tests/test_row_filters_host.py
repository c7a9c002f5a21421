"""CPU tests of per-request logits filters: the per-slot filter table's declaration (`itts_gpt_set_row_filters`), entry merging and validation
(`gpt.row_filter_entries`), what `IndexTTS2.infer_requests` and `stream_session.submit` hand to the GPT (a recording stub over the stub stages
of tests/pipeline_stubs.py), and the serving shell moving the filter kwargs out of the group key."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from indextts_amd import _lib, gpt
from tests.pipeline_stubs import StubFrontend

V, STOP = 8194, 8193


def _entries(rows, call=None, n=None, max_new=28, **kw):
    return gpt.row_filter_entries(rows, len(rows) if n is None else n, call or {}, V, STOP, max_new, **kw)


def _is_off(e):
    return ((e.min_new_tokens, e.min_length, e.no_repeat_ngram_size, e.n_suppress, e.n_begin_suppress, e.n_decay) == (0,) * 6
            and e.min_p == -1.0 and e.epsilon_cutoff == 0.0 and e.eta_cutoff == 0.0)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_refuses_a_null_handle():
    hdr = open(os.path.join(_lib.HERE, "..", "include", "indextts_hip.h")).read()
    decl = "int itts_gpt_set_row_filters(itts_gpt* h, const itts_logits_filters* entries, const int32_t* slots, int n, int n_slots);"
    assert decl in hdr and "#define ITTS_ABI_VERSION 13" in hdr
    # the call-wide block and its declaration stand as they were; the new entry follows them
    assert "/* Logits filters (v13, additive: device logits processors)" in hdr
    assert "int itts_gpt_set_logits_filters(itts_gpt* h, const itts_logits_filters* f);   /* f == NULL clears */" in hdr
    assert hdr.index("int itts_gpt_set_logits_filters(") < hdr.index("Per-slot logits filters (v13, additive") < hdr.index(decl)
    comment = hdr[hdr.index("Per-slot logits filters (v13, additive"):hdr.index(decl)]
    for word in ("OFF record", "n_slots", "ITTS_ERR_STATE", "entries == NULL", "no_repeat_ngram_size"):
        assert word in comment, word
    res, args = _lib.SIGNATURES["itts_gpt_set_row_filters"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(_lib.LogitsFilters), C.POINTER(C.c_int32), C.c_int, C.c_int]
    L = _lib.lib()
    assert L.itts_gpt_set_row_filters(None, None, None, 0, 0) == _lib.ERR_ARG          # host-only check: no GPU needed
    one = (_lib.LogitsFilters * 1)(gpt.off_filters())
    assert L.itts_gpt_set_row_filters(None, one, None, 1, 1) == _lib.ERR_ARG
    assert b"null handle" in L.itts_last_error()


# ---- merging and validation ----------------------------------------------------------------------------------------------------------------
def test_the_entrys_key_wins_and_a_missing_key_takes_the_calls_value():
    call = dict(min_new_tokens=5, suppress_tokens=[7, 9], top_k=30, do_sample=True)      # (non-filter kwargs of the call are ignored)
    e = _entries([dict(min_new_tokens=12), None, {}, dict(min_p=0.25), dict(suppress_tokens=[3])], call)
    assert [x.min_new_tokens for x in e] == [12, 5, 5, 5, 5]
    assert [x.n_suppress for x in e] == [2, 2, 2, 2, 1] and e[4].suppress_ids[0] == 3 and [e[0].suppress_ids[i] for i in range(2)] == [7, 9]
    assert [x.min_p for x in e] == [-1.0, -1.0, -1.0, 0.25, -1.0]
    # None and {} are the call-wide record's values, field for field
    wide = gpt.logits_filters(call, V, STOP, 28)
    for x in (e[1], e[2]):
        assert (x.min_new_tokens, x.min_length, x.no_repeat_ngram_size, x.decay_start, x.n_suppress, x.n_begin_suppress, x.n_decay, x.min_p) == \
               (wide.min_new_tokens, wide.min_length, wide.no_repeat_ngram_size, wide.decay_start, wide.n_suppress, wide.n_begin_suppress,
                wide.n_decay, wide.min_p)
    # a key the entry has wins whatever it holds: None is HF's default, the filter is off for that row
    e = _entries([dict(min_new_tokens=None, suppress_tokens=None), None], call)
    assert _is_off(e[0]) and e[1].min_new_tokens == 5
    # min_new_tokens over min_length, per row: the entry's min_new_tokens silences the call's min_length
    e = _entries([dict(min_new_tokens=4), None], dict(min_length=20), prompt_len=16)
    assert (e[0].min_new_tokens, e[0].min_length) == (4, 0) and (e[1].min_new_tokens, e[1].min_length) == (0, 20)
    # the decay table spans the call's steps
    e = _entries([dict(exponential_decay_length_penalty=(3, 1.5)), None])
    assert e[0].n_decay == 28 and e[0].decay_start == 3 and e[0].decay_table[3] == 0.0 and abs(e[0].decay_table[5] - 1.25) < 1e-6
    assert _is_off(e[1])


def test_hfs_off_values_build_the_off_entry():
    off = gpt.off_filters()
    assert _is_off(off) and off.decay_start == 0
    e = _entries([dict(min_new_tokens=0, min_length=0, no_repeat_ngram_size=0, epsilon_cutoff=0.0, eta_cutoff=1.0, suppress_tokens=[],
                       begin_suppress_tokens=[]), None, {}])
    assert all(_is_off(x) for x in e)
    assert not _is_off(_entries([dict(min_p=0.0)])[0])                                 # min_p = 0 is a warper HF builds: not off


def test_unknown_keys_and_bad_shapes_raise():
    with pytest.raises(ValueError, match="unknown keys") as ei:
        _entries([None, dict(top_p=0.5)])
    assert "row_filters[1]" in str(ei.value) and all(k in str(ei.value) for k in gpt._LOGITS_FILTER_KWARGS)
    with pytest.raises(ValueError, match="one entry per row"):
        _entries([None], n=2)
    with pytest.raises(ValueError, match="one entry per utterance"):
        _entries([None], n=2, num_beams=3, name="group_filters")
    with pytest.raises(TypeError, match="dict or None"):
        _entries([None, "min_p"])
    with pytest.raises(ValueError, match=r"row_filters\[1\].*min_p"):                  # HF's message, with the entry's name in front
        _entries([None, dict(min_p=1.5)])
    with pytest.raises(ValueError, match=r"row_filters\[0\].*outside the vocabulary"):
        _entries([dict(suppress_tokens=[V])])


def test_feasibility_is_checked_against_the_rows_own_cap_and_prompt():
    rows = [dict(min_new_tokens=12), dict(min_new_tokens=12)]
    assert len(_entries(rows, prompt_len=16, row_max_new=[28, 12])) == 2
    with pytest.raises(ValueError, match=r"row_filters\[1\]: Unfeasible length constraints: `min_new_tokens` \(12\)"):
        _entries(rows, prompt_len=16, row_max_new=[28, 11])
    with pytest.raises(ValueError, match=r"row_filters\[0\]: Unfeasible length constraints: `min_length` \(40\)"):
        _entries([dict(min_length=40), None], prompt_len=16, row_max_new=[20, 28])
    assert _entries([dict(min_length=40), None], prompt_len=16)[0].min_length == 40    # feasible under the call's 28 steps
    with pytest.raises(ValueError, match="Unfeasible"):                                # the call's value reaches a capped row too
        _entries([None, None], dict(min_new_tokens=12), prompt_len=16, row_max_new=[28, 5])
    with pytest.raises(ValueError, match="one entry per row"):
        _entries([None, None], row_max_new=[28])


def test_refusals_hold_per_entry():
    with pytest.raises(NotImplementedError, match=r"group_filters\[1\].*no_repeat_ngram_size"):
        _entries([None, dict(no_repeat_ngram_size=2)], num_beams=3, name="group_filters")
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):             # ... and the call's value merged into a group entry
        _entries([None], dict(no_repeat_ngram_size=2), num_beams=3, name="group_filters")
    assert _entries([dict(no_repeat_ngram_size=2)])[0].no_repeat_ngram_size == 2       # a num_beams = 1 matter
    with pytest.raises(NotImplementedError, match=r"row_filters\[0\].*multi-token"):
        _entries([dict(bad_words_ids=[[5, 6]])])
    assert _entries([dict(bad_words_ids=[[5], [STOP]])])[0].n_suppress == 1            # the [eos] word is dropped as HF drops it


def test_the_decode_entries_name_the_other_table():
    m = object.__new__(gpt.UnifiedVoice)
    m.number_mel_codes, m.stop_mel_token = V, STOP
    emb = torch.zeros(2, 15, 8)
    with pytest.raises(ValueError, match="group_filters"):
        m._filters_for({}, [None, None], None, emb, 28, 3, "generate")
    with pytest.raises(ValueError, match="row_filters"):
        m._filters_for({}, None, [None, None], emb, 28, 1, "generate")
    tab = m._filters_for(dict(min_new_tokens=3), [None, dict(min_p=0.1)], None, emb, 28, 1, "generate")
    assert isinstance(tab, gpt._FilterTable) and [e.min_new_tokens for e in tab] == [3, 3] and tab[1].min_p == pytest.approx(0.1)
    assert m._filters_for({}, None, None, emb, 28, 1, "generate") is None              # no table, no filters: nothing to install
    wide = m._filters_for(dict(min_new_tokens=3), None, None, emb, 28, 1, "generate")
    assert isinstance(wide, _lib.LogitsFilters) and not isinstance(wide, gpt._FilterTable)
    # the reference-rule prefix refuses the counted filters in an entry as it refuses them in the call
    m2 = object.__new__(gpt.UnifiedVoice)
    m2.max_mel_tokens, m2.spk_cond_mode = 30, "campplus"
    m2.prepare_gpt_inputs = lambda conds, text, langs: (None, torch.zeros(2, 15, 8), torch.ones(2, 16))
    for key, val in (("min_new_tokens", 3), ("begin_suppress_tokens", [1]), ("exponential_decay_length_penalty", (2, 1.1))):
        with pytest.raises(ValueError, match="input_tokens"):
            m2._prepare_inference(None, torch.zeros(2, 4), None, None, None, None, torch.tensor([5, 6]), 1, 20, False, 0.9, torch.zeros(2, 3, 8),
                                  dict(row_filters=[None, {key: val}]))


# ---- infer_requests over a recording GPT stub --------------------------------------------------------------------------------------------
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

    def _record(self, name, kw):
        self.calls.append((name, kw))
        raise _Recorded

    def inference_speech(self, *a, **kw):
        self._record("inference_speech", kw)

    def inference_speech_inflight(self, *a, **kw):
        self._record("inference_speech_inflight", kw)

    def inference_speech_inflight_beams(self, *a, **kw):
        self._record("inference_speech_inflight_beams", kw)


def _pipeline():
    from indextts_amd.infer_v2_5 import IndexTTS2
    from indextts_amd.serving import SpeakerCache
    t = object.__new__(IndexTTS2)
    t.frontend, t.gpt, t.device = StubFrontend(8), _StubGPT(), "cpu"
    t.speaker_cache = SpeakerCache(lambda a: t.frontend.speaker_bundle(a))
    t.emotion_cache = SpeakerCache(lambda a: t.frontend.emo_cond(a))
    t.prompt_batching = False
    return t


REQS = [dict(spk_audio_prompt="a.wav", text="one. two", lang="en", min_new_tokens=20, seed=11),
        dict(spk_audio_prompt="b.wav", text="three", lang="en", best_of=2),
        dict(spk_audio_prompt="a.wav", text="four", lang="en", suppress_tokens=[5, 6], min_p=0.2)]


def _call(t, reqs, **kw):
    with pytest.raises(_Recorded):
        t.infer_requests(reqs, **kw)
    return t.gpt.calls[-1]


def test_differing_request_filters_reach_the_gpt_as_one_entry_per_row():
    name, kw = _call(_pipeline(), REQS, num_beams=1, max_mel_tokens=24, min_new_tokens=3, eta_cutoff=0.1)
    assert name == "inference_speech" and kw["min_new_tokens"] == 3 and kw["eta_cutoff"] == 0.1      # the call's values stay the defaults
    # rows: request 0's two segments, request 1's two candidates, request 2 -- segments and candidates share the request's entry
    assert kw["row_filters"] == [dict(min_new_tokens=20)] * 2 + [{}] * 2 + [dict(suppress_tokens=[5, 6], min_p=0.2)]
    assert len(kw["row_sampling"]) == len(kw["row_max_new"]) == 5 and "group_filters" not in kw
    e = gpt.row_filter_entries(kw["row_filters"], 5, kw, V, STOP, 24)                  # and the engine's builder takes them over the call's kwargs
    assert [x.min_new_tokens for x in e] == [20, 20, 3, 3, 3] and all(x.eta_cutoff == pytest.approx(0.1) for x in e)
    assert [x.n_suppress for x in e] == [0, 0, 0, 0, 2]
    # more rows than decode slots: the in-flight path gets the same entries
    name, kw = _call(_pipeline(), REQS, num_beams=1, max_mel_tokens=24, inflight_slots=2)
    assert name == "inference_speech_inflight" and kw["slots"] == 2 and len(kw["row_filters"]) == 5
    assert kw["row_filters"][0] == dict(min_new_tokens=20) and kw["row_filters"][2] == {}


def test_equal_request_filters_take_the_call_wide_path():
    same = [dict(spk_audio_prompt="a.wav", text="x", lang="en", min_new_tokens=7), dict(spk_audio_prompt="b.wav", text="y", lang="en", min_new_tokens=7)]
    name, kw = _call(_pipeline(), same, num_beams=1, max_mel_tokens=24, min_new_tokens=3, min_p=0.1)
    assert "row_filters" not in kw and "group_filters" not in kw and kw["min_new_tokens"] == 7 and kw["min_p"] == 0.1
    # a request key that restates the call's value changes nothing either; no request filters at all: the kwargs of a call without the feature
    mixed = [dict(same[0], min_new_tokens=3), dict(spk_audio_prompt="b.wav", text="y", lang="en")]
    name, kw = _call(_pipeline(), mixed, num_beams=1, max_mel_tokens=24, min_new_tokens=3)
    assert "row_filters" not in kw and kw["min_new_tokens"] == 3
    plain = [dict(spk_audio_prompt="a.wav", text="x", lang="en"), dict(spk_audio_prompt="b.wav", text="y", lang="en")]
    name, kw = _call(_pipeline(), plain, num_beams=1, max_mel_tokens=24)
    assert not set(kw) & (set(gpt._LOGITS_FILTER_KWARGS) | {"row_filters", "group_filters"})
    # beams, shared settings, equal filters: today's scalar beam call with the filters call-wide
    name, kw = _call(_pipeline(), same, max_mel_tokens=24)
    assert kw["num_beams"] == 3 and kw["min_new_tokens"] == 7 and "group_filters" not in kw and "group_sampling" not in kw


def test_beams_own_get_group_filters_and_shared_beams_refuse():
    reqs = [dict(r) for r in REQS]
    reqs[1].pop("best_of")
    name, kw = _call(_pipeline(), reqs, beam_settings="own", max_mel_tokens=24)
    assert name == "inference_speech" and kw["num_beams"] == 3 and "row_filters" not in kw
    assert kw["group_filters"] == [dict(min_new_tokens=20)] * 2 + [{}] + [dict(suppress_tokens=[5, 6], min_p=0.2)]
    assert len(kw["group_sampling"]) == 4
    name, kw = _call(_pipeline(), reqs, beam_settings="own", max_mel_tokens=24, inflight_beam_slots=2)
    assert name == "inference_speech_inflight_beams" and len(kw["group_filters"]) == 4
    t = _pipeline()
    with pytest.raises(ValueError, match="logits filters") as ei:
        t.infer_requests(reqs, max_mel_tokens=24)
    assert "beam_settings" in str(ei.value) and "min_new_tokens" in str(ei.value) and not t.gpt.calls
    with pytest.raises(ValueError, match="unknown keys"):
        _pipeline().infer_requests([dict(REQS[0], min_tokens=3)], num_beams=1)


def test_stream_session_submit_accepts_the_keys():
    from tests.test_stream_session_host import _cpu_tts
    tts = _cpu_tts()
    sess = tts.stream_session(slots=2, chunk_size=8, overlap_size=2, max_mel_tokens=24, cfm_noise="global", min_new_tokens=4)
    sid = sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", min_new_tokens=9, suppress_tokens=[3]))
    sid2 = sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en"))
    items = [w[1] for w in sess._waiting]
    assert (sid, sid2) == (0, 1) and items[0].filters == dict(min_new_tokens=9, suppress_tokens=[3]) and items[1].filters == {}
    with pytest.raises(ValueError, match="unknown keys"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", min_tokens=9))
    # a bad VALUE is the submitting caller's error too, before anything is queued: HF's message, and feasibility against the stream's own cap
    with pytest.raises(ValueError, match=r"request 2: filters\[0\].*min_p"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", min_p=1.5))
    with pytest.raises(ValueError, match="Unfeasible length constraints"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", min_new_tokens=9, max_mel_tokens=8))
    with pytest.raises(ValueError, match="Unfeasible length constraints"):             # the session's own value reaches a capped stream
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", max_mel_tokens=3))
    with pytest.raises(NotImplementedError, match="multi-token"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", bad_words_ids=[[4, 5]]))
    assert len(sess._waiting) == 2
    assert sess.cancel(sid) and sess.cancel(sid2)
    sess.step()
    sess.close()


# ---- the serving shell ---------------------------------------------------------------------------------------------------------------------
class _FakeTTS:
    def __init__(self):
        self.request_calls = []

    def infer_requests(self, requests, **defaults):
        self.request_calls.append(([dict(r) for r in requests], dict(defaults)))
        return [(22050, np.full((len(r["text"]), 1), 1, dtype=np.int16)) for r in requests]


def test_the_serving_shells_filter_keys_are_the_engines():
    from indextts_amd import serving
    assert set(serving.PER_REQUEST_FILTERS) == set(gpt._LOGITS_FILTER_KWARGS) and len(serving.PER_REQUEST_FILTERS) == len(gpt._LOGITS_FILTER_KWARGS) == 10


def _batch(tts, request_filters, **wide):
    from indextts_amd.serving import DynamicBatcher
    b = DynamicBatcher(tts, max_batch=2, max_wait_ms=20, mixed=True, **({} if request_filters is None else dict(request_filters=request_filters)))
    futs = [b.submit(b"A", "tt", "en", min_new_tokens=20, **wide), b.submit(b"B", "t", "en", **wide)]
    for f in futs:
        f.result(timeout=10)
    b.close()
    return sorted(b.batches)


def test_dynamic_batcher_moves_the_filters_out_of_the_group_key_on_request():
    tts = _FakeTTS()
    assert _batch(tts, True, num_beams=1, min_p=0.1) == [2]                            # one batch: the filters travel with the requests
    (reqs, defaults), = tts.request_calls
    assert defaults == dict(num_beams=1) and reqs[0]["min_new_tokens"] == 20 and reqs[0]["min_p"] == 0.1
    assert "min_new_tokens" not in reqs[1] and reqs[1]["min_p"] == 0.1
    for flag in (None, False):                                                         # the default keeps today's grouping exactly
        tts = _FakeTTS()
        assert _batch(tts, flag, num_beams=1) == [1, 1]
        assert sorted(d.get("min_new_tokens", 0) for _, d in tts.request_calls) == [0, 20]
        assert all("min_new_tokens" not in r for rs, _ in tts.request_calls for r in rs)
    tts = _FakeTTS()                                                                   # shared beam settings: the filters stay in the key
    assert _batch(tts, True) == [1, 1]
    tts = _FakeTTS()
    assert _batch(tts, True, beam_settings="own") == [2]


def test_synthesize_tasks_carries_a_tasks_filters_on_request(tmp_path):
    from indextts_amd.serving import synthesize_tasks
    tasks = [dict(voice_path="v0.wav", text="xx", output_path=tmp_path / "0.wav", min_new_tokens=20),
             dict(voice_path="v1.wav", text="xxx", output_path=tmp_path / "1.wav")]
    tts = _FakeTTS()
    synthesize_tasks(tts, tasks, lang="en", mixed=True, request_filters=True, num_beams=1, min_p=0.1)
    (reqs, defaults), = tts.request_calls
    assert defaults == dict(num_beams=1, min_p=0.1) and reqs[0]["min_new_tokens"] == 20 and "min_new_tokens" not in reqs[1]
    tts = _FakeTTS()
    synthesize_tasks(tts, tasks, lang="en", mixed=True, num_beams=1)
    assert all("min_new_tokens" not in r for r in tts.request_calls[0][0])             # the default: as today
