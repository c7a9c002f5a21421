"""Host side of the ragged prompt batch (no GPU): the four v13 entries in the header and the ctypes table, the pure head-grouping function of
`CAMPPlus.forward_ragged`, `SpeakerCache.get_or_compute_many`, the `Frontend.speaker_bundles` default, and the cache warm-up of
`infer_requests(prompt_batching=True)` on the stub front end of tests/pipeline_stubs.py."""
import os
import re

import pytest
import torch

from indextts_amd import _lib
from indextts_amd.campplus import DEFAULT_COL_BUDGET, head_col_bytes, head_groups
from indextts_amd.infer_v2_5 import Frontend, IndexTTS2
from indextts_amd.serving import SpeakerCache
from tests.pipeline_stubs import StubFrontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("itts_tok_ctxpool_seq_forward", "itts_tok_statspool_seq_forward", "itts_tok_gather_conv1d_seq_forward", "itts_tok_gather_conv2d_seq_forward")


def test_header_declares_the_entries_as_v13_additions():
    hdr = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert "#define ITTS_ABI_VERSION 13" in hdr and _lib.ABI_VERSION == 13
    at = hdr.index("(v13, additive: ragged prompt batch)")
    block = hdr[at: hdr.index("prompt-audio front end", at)]
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\(", block), f"{name} is not declared in the ragged prompt batch block"
        assert name in _lib.SIGNATURES, f"{name} is missing from _lib.SIGNATURES"
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", block).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), f"{name}: the ctypes signature and the header disagree on the argument count"
    # every entry's comment names the reference lines it replaces
    for cite in ("layers.py:93-110", "layers.py:26-37", "layers.py:55-61", "layers.py:81-87", "DTDNN.py:21,27", "layers.py:223-246", "DTDNN.py:111-116"):
        assert cite in block, cite
    # the single-sequence entries are still declared as they were
    assert "int itts_tok_ctxpool_forward(const float* h, float* out, int n, int C, int seg_len, void* stream);" in hdr
    assert "int itts_tok_statspool_forward(const float* x, float* out, int n, int C, void* stream);" in hdr


# ---- head grouping ------------------------------------------------------------------------------------------------------------------------------
def test_head_col_bytes_is_the_widest_column_matrix():
    # 80 bins: conv1 builds [80 T][9], the first residual block [40 T][288] -- the widest --, the later ones [20 T][288], conv2 [10 T][288]
    assert head_col_bytes(1) == 4 * 40 * 288 and head_col_bytes(1500) == 1500 * head_col_bytes(1)
    assert head_col_bytes(7, feat_dim=1) == 4 * 7 * 288                  # one bin: every conv keeps height 1


@pytest.mark.parametrize("lens,budget_frames", [((100, 200, 300, 50, 50, 700, 10), 400), ((5,), 1), ((900, 900, 900), 100), ((4, 4, 4, 4), 8),
                                                ((10, 20, 30), 10 ** 6)])
def test_head_groups(lens, budget_frames):
    budget = head_col_bytes(budget_frames)
    groups = head_groups(lens, budget)
    assert [i for g in groups for i in g] == list(range(len(lens)))      # order preserved, every sequence exactly once
    for g in groups:
        assert g
        if len(g) > 1:
            assert head_col_bytes(sum(lens[i] for i in g)) <= budget     # groups stay under the budget ...
        elif lens[g[0]] > budget_frames:
            assert len(g) == 1                                           # ... but a single sequence over it forms a group of its own
    for a, b in zip(groups, groups[1:]):                                  # greedy: the next group's first sequence did not fit
        assert head_col_bytes(sum(lens[i] for i in a) + lens[b[0]]) > budget


def test_head_groups_examples():
    b = head_col_bytes(400)
    assert head_groups((100, 200, 300, 50, 50, 700, 10), b) == [[0, 1], [2, 3, 4], [5], [6]]
    assert head_groups((), b) == []
    assert head_groups((1500,) * 4) == [[0, 1, 2, 3]] and DEFAULT_COL_BUDGET == 2 << 30
    assert len(head_groups((1500,) * 64)) == 3                            # 64 prompts of 15 s: 31 fit 2 GiB


# ---- SpeakerCache.get_or_compute_many ---------------------------------------------------------------------------------------------------------------
def _many(calls):
    def compute_many(audios):
        calls.append(list(audios))
        return [("bundle", a) for a in audios]
    return compute_many


def test_get_or_compute_many_one_call_for_the_distinct_misses():
    calls, single = [], []
    c = SpeakerCache(lambda a: single.append(a) or ("bundle", a))
    out = c.get_or_compute_many(["a", "b", "a", "c", "b"], _many(calls))
    assert calls == [["a", "b", "c"]] and single == []                    # ONE call, distinct prompts in first-appearance order
    assert out == [("bundle", k) for k in ("a", "b", "a", "c", "b")]       # input order; a duplicate gets the one computed value
    assert out[0] is out[2]
    assert (c.misses, c.hits) == (3, 2)
    # the counters are those of a loop of get_or_compute over the same list
    ref = SpeakerCache(lambda a: ("bundle", a))
    for a in ["a", "b", "a", "c", "b"]:
        ref.get_or_compute(a)
    assert (ref.misses, ref.hits) == (c.misses, c.hits)
    # all hit: no call
    out2 = c.get_or_compute_many(["c", "a"], _many(calls))
    assert len(calls) == 1 and out2 == [("bundle", "c"), ("bundle", "a")] and (c.misses, c.hits) == (3, 4)
    # partly cached: only the cold ones are computed; a later get_or_compute hits
    out3 = c.get_or_compute_many(["d", "a", b"raw"], _many(calls))
    assert calls[-1] == ["d", b"raw"] and out3[1] == ("bundle", "a") and (c.misses, c.hits) == (5, 5)
    assert c.get_or_compute("d") == ("bundle", "d") and single == [] and c.hits == 6
    assert c.get_or_compute_many([], _many(calls)) == [] and len(calls) == 2


def test_get_or_compute_many_keeps_the_lru_bound():
    calls = []
    c = SpeakerCache(lambda a: ("bundle", a), max_size=3)
    c.get_or_compute_many(["a", "b"], _many(calls))
    c.get_or_compute_many(["a", "c", "d"], _many(calls))                   # "a" was touched: "b" is the oldest
    assert calls == [["a", "b"], ["c", "d"]] and list(c._d) == [SpeakerCache.key_of(k) for k in ("a", "c", "d")]
    out = c.get_or_compute_many(["e", "f", "g", "h"], _many(calls))        # more cold prompts than the cache holds: all returned, the last 3 kept
    assert out == [("bundle", k) for k in "efgh"] and len(c._d) == 3 and list(c._d) == [SpeakerCache.key_of(k) for k in "fgh"]
    with pytest.raises(RuntimeError):
        c.get_or_compute_many(["x", "y"], lambda audios: [("bundle", audios[0])])


# ---- front ends ---------------------------------------------------------------------------------------------------------------------------------
def test_frontend_default_loops_speaker_bundle():
    fe = StubFrontend(64)
    bundles = fe.speaker_bundles(["p.wav", "q.wav", "p.wav"])
    assert fe.calls == [("speaker", "p.wav"), ("speaker", "q.wav"), ("speaker", "p.wav")]
    assert len(bundles) == 3 and set(bundles[0]) == {"style", "spk_cond_emb", "ref_mel", "prompt_condition"}
    fe.calls.clear()
    assert len(fe.emo_conds(["e.wav"])) == 1 and fe.calls == [("emo", "e.wav")]
    assert Frontend.speaker_bundles(fe, []) == []


class _Gpt:
    cond_encoders = None
    n_text_pos = 602

    def conds_latent(self, style, emovec):
        return torch.zeros(1, 1, 3, 8)


REQUESTS = [dict(spk_audio_prompt="v1.wav", text="a.", lang="en"),
            dict(spk_audio_prompt="v2.wav", text="b.", lang="en", emo_audio_prompt="e1.wav"),
            dict(spk_audio_prompt="v1.wav", text="c.", lang="en", emo_audio_prompt="e1.wav"),
            dict(spk_audio_prompt="v3.wav", text="d.", lang="en", emo_audio_prompt="e2.wav", emo_vector=[0.1] * 8)]


def _tts(fe):
    return IndexTTS2(cfg={"gpt": {"stop_mel_token": 8193}}, device="cpu", frontend=fe, gpt=_Gpt(), bigvgan=object())


class _Stop(Exception):
    pass


def _run_until_text(tts, **kw):
    """infer_requests up to the end of the request loop: the stub's text_segments of the LAST request raises, after every request's conditioning"""
    fe, n = tts.frontend, [0]
    segs = fe.text_segments

    def text_segments(*a):
        n[0] += 1
        if n[0] == len(REQUESTS):
            raise _Stop
        return segs(*a)
    fe.text_segments = text_segments
    with pytest.raises(_Stop):
        tts.infer_requests(REQUESTS, num_beams=1, **kw)
    fe.text_segments = segs


def test_prompt_batching_warms_the_caches_through_one_call():
    fe = StubFrontend(64)
    batched = []
    fe.speaker_bundles = lambda prompts: batched.append(("speakers", list(prompts))) or [_bundle(fe) for _ in prompts]
    fe.emo_conds = lambda prompts: batched.append(("emos", list(prompts))) or [torch.zeros(1, 4, 1024) for _ in prompts]
    tts = _tts(fe)
    assert tts.prompt_batching is False
    _run_until_text(tts, prompt_batching=True)
    # ONE speaker_bundles call with the distinct prompts in first-appearance order; the emotion prompts likewise (a request without one -- or with
    # an emotion vector -- conditions on its speaker prompt); speaker_bundle / emo_cond are never called
    assert batched == [("speakers", ["v1.wav", "v2.wav", "v3.wav"]), ("emos", ["v1.wav", "e1.wav", "v3.wav"])]
    assert fe.calls == []
    assert (tts.speaker_cache.misses, tts.emotion_cache.misses) == (3, 3)
    # a second call finds everything cached: no front-end call at all
    _run_until_text(tts, prompt_batching=True)
    assert len(batched) == 2 and fe.calls == []


def _bundle(fe):
    return dict(style=fe.style, spk_cond_emb=torch.zeros(1, 4, 1024), ref_mel=torch.zeros(1, 80, 5), prompt_condition=torch.zeros(1, 5, 512))


def test_without_prompt_batching_the_call_pattern_is_unchanged():
    expected = [("speaker", "v1.wav"), ("emo", "v1.wav"), ("speaker", "v2.wav"), ("emo", "e1.wav"), ("speaker", "v3.wav"), ("emo", "v3.wav")]
    for kw in ({}, dict(prompt_batching=False)):
        fe = StubFrontend(64)
        fe.speaker_bundles = fe.emo_conds = lambda prompts: pytest.fail("the batched front-end call ran with prompt_batching off")
        _run_until_text(_tts(fe), **kw)
        assert fe.calls == expected
    # the attribute is the default of the kwarg, and the kwarg wins
    fe = StubFrontend(64)
    tts = _tts(fe)
    tts.prompt_batching = True
    _run_until_text(tts)
    assert fe.calls == [("speaker", "v1.wav"), ("speaker", "v2.wav"), ("speaker", "v3.wav"), ("emo", "v1.wav"), ("emo", "e1.wav"), ("emo", "v3.wav")]
    fe.calls.clear()
    tts2 = _tts(fe)
    tts2.prompt_batching = True
    _run_until_text(tts2, prompt_batching=False)
    assert fe.calls == expected


def test_batcher_and_batch_file_pass_the_option_through():
    from indextts_amd.serving import DynamicBatcher, synthesize_tasks
    seen = []

    class T:
        def infer_requests(self, reqs, **kw):
            seen.append(kw)
            return [None] * len(reqs)
    b = DynamicBatcher(T(), max_batch=2, max_wait_ms=1.0, mixed=True)
    f = b.submit("v.wav", "a.", "en", num_beams=1, prompt_batching=True)
    assert f.result(timeout=30) is None
    b.close()
    assert seen[-1].get("prompt_batching") is True
    synthesize_tasks(T(), [dict(voice_path="v.wav", text="a.", output_path="unused.wav")], lang="en", mixed=True, prompt_batching=True)
    assert seen[-1].get("prompt_batching") is True
