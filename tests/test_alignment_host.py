"""CPU tests of the text-attention export and the timestamps: the two C entries' declarations (`itts_gpt_set_alignment`,
`itts_gpt_attention_align_forward`), the `TokenAlignment` record -- its monotonic alignment search against an exhaustive enumeration --, the
timestamp arithmetic of `IndexTTS2.infer_requests(timestamps=True)` over stand-in stages (a stub GPT that returns scripted codes and a
scripted attention), the unit case matrix of tests/align_ref.py, and the refusals.  The kernel is held to f64 in tests/test_gpu_align_matrix.py."""
import os

import pytest
import torch

from indextts_amd import _lib, gpt
from tests import align_ref as R
from tests.test_pipeline_cpu import FakeVoc
from tests.test_token_scores_host import RecordingFrontend

STOP = 8193
UP = 256
SPC = 2 * 1.72 * UP                      # samples per code at duration_factor 1


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(_lib.HERE, "..", "include", "indextts_hip.h")).read()
    assert "int itts_gpt_set_alignment(itts_gpt* h, const int32_t* pairs, int n_pairs, const int32_t* span, float* out, int n, int max_new, int text_cap);" in hdr
    assert "v13, additive: alignment export" in hdr and "#define ITTS_ABI_VERSION 13" in hdr
    comment = hdr[hdr.index("v13, additive: alignment export"):hdr.index("int itts_gpt_set_alignment(")]
    for word in ("output_attentions", "F64", "finished", "zero-fills", "graph", "ITTS_ERR_STATE", "never written"):
        assert word in comment, word
    assert "int itts_gpt_attention_align_forward(const float* q, const void* kcache, float* out, const int32_t* span" in hdr
    L = _lib.lib()
    for name in ("itts_gpt_set_alignment", "itts_gpt_attention_align_forward"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.itts_abi_version() == 13
    assert L.itts_gpt_set_alignment(None, None, 0, None, None, 0, 0, 0) == _lib.ERR_ARG              # host-only checks: no GPU needed
    assert L.itts_gpt_attention_align_forward(*([None] * 5), 1, *([None] * 9), 1, 2, 8, 1, 4, 8, 0, None) == _lib.ERR_ARG
    names = [L.itts_attention_path_name(i).decode() for i in range(L.itts_attention_path_count())]
    assert not any("align" in n for n in names), "the export has a launcher of its own: it is not one of launch_attention's paths"


def test_path_equals_exhaustive_enumeration():
    g = torch.Generator().manual_seed(5)
    checked = 0
    for n in range(1, 7):
        for T in range(1, min(n, 4) + 1):
            for _ in range(6):
                a = torch.rand(n, T, generator=g, dtype=torch.float64) ** 3 + 1e-3
                a = a / a.sum(1, keepdim=True)
                logp = torch.log(a + gpt.TokenAlignment.EPS)
                score, path = R.exhaustive_best_path(logp.tolist())
                got = gpt.monotonic_path(logp.numpy())
                assert got == path, (n, T, got, path)
                assert got[0] == 0 and got[-1] == T - 1 and all(0 <= b - a_ <= 1 for a_, b in zip(got, got[1:]))
                al = gpt.TokenAlignment(a.float()[None, :, None, :], [T], [n])
                spans = al.path(0).tolist()
                assert spans == [[path.index(j), len(path) - path[::-1].index(j)] for j in range(T)]
                checked += 1
    assert checked >= 100
    with pytest.raises(ValueError):
        gpt.monotonic_path(torch.zeros(2, 3).numpy())


def _staircase(path, T, K=2, pad_rows=0, pad_cols=0):
    n = len(path)
    a = torch.zeros(1, n + pad_rows, K, T + pad_cols)
    for i, j in enumerate(path):
        a[0, i, :, j] = 1.0
    return a


def test_staircase_gives_its_exact_spans_and_monotonicity_one():
    path = [0, 0, 1, 2, 2, 2, 3]
    al = gpt.TokenAlignment(_staircase(path, 4, pad_rows=3, pad_cols=4), [4], [len(path)])
    assert al.path(0).tolist() == [[0, 2], [2, 3], [3, 6], [6, 7]]
    assert al.path(0, "max").tolist() == al.path(0, 1).tolist() == al.path(0).tolist()
    assert al.monotonicity().tolist() == [[1.0, 1.0]]
    # row 0 of a real export is zero (code 0 comes from the prefill): still pinned to text position 0
    a = _staircase(path, 4)
    a[0, 0] = 0
    assert gpt.TokenAlignment(a, [4], [7]).path(0).tolist() == [[0, 2], [2, 3], [3, 6], [6, 7]]
    # a sharp diagonal
    assert gpt.TokenAlignment(_staircase([0, 1, 2, 3, 4], 5), [5], [5]).path(0).tolist() == [[i, i + 1] for i in range(5)]
    # fewer codes than text positions: one code each, the rest empty at the end
    assert gpt.TokenAlignment(_staircase([0, 1], 4), [4], [2]).path(0).tolist() == [[0, 1], [1, 2], [2, 2], [2, 2]]
    # n_codes restricts the codes (the pipeline renders the codes before the stop token)
    assert al.path(0, n_codes=6).tolist() == [[0, 2], [2, 3], [3, 5], [5, 6]]
    # a head that ignores the text order scores about 1 / T
    flat = gpt.TokenAlignment(torch.full((1, 12, 1, 4), 0.25), [4], [12]).monotonicity()
    assert abs(float(flat[0, 0]) - 0.25) < 1e-12
    with pytest.raises(ValueError):
        al.path(0, "median")
    with pytest.raises(ValueError):
        gpt.TokenAlignment(torch.zeros(2, 3, 4), [1, 1], [1, 1])
    st = gpt.TokenAlignment.stack([al.row(0), gpt.TokenAlignment(_staircase([0, 1], 2), [2], [2])])
    assert st.attn.shape == (2, 10, 2, 8) and st.text_lens.tolist() == [4, 2] and st.path(1).tolist() == [[0, 1], [1, 2]]


def test_segment_timestamps_arithmetic():
    from indextts_amd.infer_v2_5 import IndexTTS2
    f = IndexTTS2.segment_timestamps
    spans = [[0, 2], [2, 3], [3, 5], [5, 6]]                # [start] [id 7] [id 8] [stop]
    out = f(spans, [7, 8], 6, 100000, SPC, 0)
    assert out == [dict(text_id=7, start=0.0, end=3 * SPC / 22050), dict(text_id=8, start=3 * SPC / 22050, end=100000 / 22050)]
    out = f(spans, [7, 8], 6, 2000, SPC * 1.25, 500)        # clipped at the rendered length; the offset of earlier segments added
    assert out == [dict(text_id=7, start=500 / 22050, end=2500 / 22050), dict(text_id=8, start=2500 / 22050, end=2500 / 22050)]
    assert f(spans, [], 6, 2000, SPC) == []


# ---- infer_requests over stand-in stages -------------------------------------------------------------------------------------------------
class AlignedGPT:
    """`inference_speech` returns `n_codes(row)` codes per row and leaves a staircase `last_alignment`: text position j of a row with T
    positions holds codes [j * n // T, (j + 1) * n // T)"""
    n_text_pos, layers, heads, start_text_token, stop_text_token = 42, 3, 2, 0, 1

    def __init__(self, n_codes=None, candidates=None):
        self.calls, self.last_scores, self.last_alignment = [], None, None
        self.n_codes = n_codes or (lambda text_len, stream: 2 * text_len)
        self.candidates = candidates or {}

    def conds_latent(self, style, emo_vec):
        return torch.zeros(1, 3, 64), None

    @staticmethod
    def _seed(seed, do_sample, uniforms):
        return 7 if seed is None else int(seed)

    def inference_speech(self, cond, text, langs, **kw):
        self.calls.append(("inference_speech", text.clone(), kw))
        T = [int(((t != 0) & (t != 1)).sum()) + 2 for t in text]
        n = [self.n_codes(T[b], e["stream"]) for b, e in enumerate(kw["row_sampling"])]
        W = max(n) + 1
        codes = torch.full((len(n), W), STOP, dtype=torch.long)
        attn = torch.zeros(len(n), W, len(kw.get("alignment_heads") or [0]), max(T))
        for b in range(len(n)):
            codes[b, : n[b]] = 100 + torch.arange(n[b])
            for i in range(1, n[b] + 1):                    # (row n[b] is the stop token's)
                attn[b, i, :, min(T[b] - 1, i * T[b] // n[b])] = 1.0
        self.last_alignment = gpt.TokenAlignment(attn, T, [v + 1 for v in n]) if kw.get("alignment_heads") is not None else None
        self.last_scores = None
        if kw.get("token_scores"):
            lm = torch.zeros(len(n), W)
            for b, e in enumerate(kw["row_sampling"]):
                lm[b, : n[b] + 1] = self.candidates.get(e["stream"], -1.0)
            self.last_scores = gpt.TokenScores(lm, lm.clone(), [v + 1 for v in n], [True] * len(n))
        return codes, None

    def inference_speech_inflight(self, cond, text, langs, slots=8, **kw):
        kw.pop("chunk_tokens", None), kw.pop("min_free", None)
        out = self.inference_speech(cond, text, langs, **kw)
        self.calls[-1] = ("inference_speech_inflight",) + self.calls[-1][1:]
        return out


def _tts(**kw):
    from indextts_amd.infer_v2_5 import IndexTTS2
    return IndexTTS2(cfg={"gpt": {"stop_mel_token": STOP}}, device="cpu", frontend=RecordingFrontend(64), gpt=AlignedGPT(**kw), bigvgan=FakeVoc())


HEADS = [(2, 0), (0, 1)]


def _expected_segment(n_ids, n_codes, dur, offset, rendered):
    """the staircase of AlignedGPT over T = n_ids + 2 positions, by the timing rule"""
    T = n_ids + 2
    pos = [0] + [min(T - 1, i * T // n_codes) for i in range(1, n_codes)]          # codes 0 .. n_codes - 1 (code 0's row is zero: pinned to 0)
    pos[-1] = T - 1                                                                 # the last code is pinned to the last position
    out = []
    for j in range(1, n_ids + 1):
        own = [i for i, p in enumerate(pos) if p == j]
        a = 0.0 if j == 1 else min(rendered, (own[0] if own else n_codes) * SPC * dur)
        b = rendered if j == n_ids else min(rendered, ((own[-1] + 1) if own else n_codes) * SPC * dur)
        out.append(((offset + a) / 22050, (offset + b) / 22050))
    return out


def test_timestamps_two_segments_duration_factor_silence_and_clipping():
    t = _tts()
    reqs = [dict(spk_audio_prompt="a.wav", text="abcd. efghijk", lang="en", seed=1, duration_factor=1.25),
            dict(spk_audio_prompt="b.wav", text="xyz", lang="en", seed=2)]
    outs = t.infer_requests(reqs, num_beams=1, max_mel_tokens=40, timestamps=True, alignment_heads=HEADS, interval_silence=100)
    (name, text, kw), = t.gpt.calls
    assert name == "inference_speech" and kw["alignment_heads"] == HEADS and "timestamps" not in kw
    ts = t.last_timestamps
    assert [len(r) for r in ts] == [2, 1]
    sil = int(22050 * 100 / 1000.0)
    # the stub frontend renders 2 * duration_factor frames per code: fewer than the rule's 2 * 1.72 -> the later tokens clip at the rendered end
    offset = 0
    for seg, n_ids in zip(ts[0], (4, 7)):
        n_codes = 2 * (n_ids + 2)
        rendered = int(n_codes * 2 * 1.25) * UP
        want = _expected_segment(n_ids, n_codes, 1.25, offset, rendered)
        assert [e["text_id"] for e in seg] == [int(v) for v in t.frontend.text_segments("abcd. efghijk", "en", 120, True, 42)[0 if n_ids == 4 else 1][:-1]]
        for e, (a, b) in zip(seg, want):
            assert e["start"] == pytest.approx(a, abs=1e-12) and e["end"] == pytest.approx(b, abs=1e-12), (seg, want)
        assert seg[-1]["end"] == pytest.approx((offset + rendered) / 22050) and seg[0]["start"] == pytest.approx(offset / 22050)
        assert any(e["end"] == pytest.approx((offset + rendered) / 22050) for e in seg[:-1]), "the clipping case must occur"
        offset += rendered + sil
    assert outs[0][1].shape[0] == offset - sil               # the request's waveform: its segments and one silence between them
    seg = ts[1][0]
    assert seg[0]["start"] == 0.0 and seg[-1]["end"] == pytest.approx(outs[1][1].shape[0] / 22050)
    flat = [e for s in ts[0] for e in s]
    assert all(a["end"] <= b["start"] + 1e-12 for a, b in zip(flat, flat[1:]))
    # without silence the second segment starts where the first one ends
    t.infer_requests(reqs[:1], num_beams=1, max_mel_tokens=40, timestamps=True, alignment_heads=HEADS, interval_silence=0)
    assert t.last_timestamps[0][1][0]["start"] == pytest.approx(t.last_timestamps[0][0][-1]["end"])
    # the attribute serves where the kwarg is missing; without timestamps nothing is asked of the engine
    t.alignment_heads = HEADS
    t.infer_requests(reqs, num_beams=1, max_mel_tokens=40, timestamps=True, interval_silence=100)
    assert t.last_timestamps == ts
    t.infer_requests(reqs, num_beams=1, max_mel_tokens=40)
    assert t.last_timestamps is None and "alignment_heads" not in t.gpt.calls[-1][2]


def test_timestamps_report_the_best_of_winner():
    C1 = 1 << 16
    # candidate 1 (stream C1) wins on its mean log-probability and is LONGER: its alignment, not candidate 0's, must be reported
    t = _tts(n_codes=lambda T, stream: 3 * T if stream >= C1 else 2 * T, candidates={0: -2.0, C1: -0.5})
    req = dict(spk_audio_prompt="a.wav", text="abcd", lang="en", seed=1, best_of=2)
    out = t.infer_requests([req], num_beams=1, max_mel_tokens=40, timestamps=True, alignment_heads=HEADS)
    assert t.last_scores[0][0]["chosen"] == 1
    n_codes = 18
    rendered = n_codes * 2 * UP
    assert out[0][1].shape[0] == rendered
    want = _expected_segment(4, n_codes, 1.0, 0, rendered)
    for e, (a, b) in zip(t.last_timestamps[0][0], want):
        assert e["start"] == pytest.approx(a, abs=1e-12) and e["end"] == pytest.approx(b, abs=1e-12)
    t2 = _tts()
    t2.infer_requests([dict(req, best_of=1)], num_beams=1, max_mel_tokens=40, timestamps=True, alignment_heads=HEADS)
    assert t2.last_timestamps != t.last_timestamps
    # the in-flight path carries it too
    t3 = _tts()
    reqs = [dict(spk_audio_prompt="a.wav", text=x, lang="en", seed=i) for i, x in enumerate(("abcd", "efg", "hijkl"))]
    t3.infer_requests(reqs, num_beams=1, max_mel_tokens=40, timestamps=True, alignment_heads=HEADS)
    base = t3.last_timestamps
    t3.infer_requests(reqs, num_beams=1, max_mel_tokens=40, timestamps=True, alignment_heads=HEADS, inflight_slots=2)
    assert t3.gpt.calls[-1][0] == "inference_speech_inflight" and t3.last_timestamps == base


def test_refusals_come_before_any_engine_work():
    req = dict(spk_audio_prompt="a.wav", text="hello", lang="en")
    t = _tts()
    with pytest.raises(ValueError, match="alignment_heads"):                         # no default list is shipped
        t.infer_requests([req], num_beams=1, timestamps=True)
    with pytest.raises(ValueError, match="num_beams"):
        t.infer_requests([req], timestamps=True, alignment_heads=HEADS)            # (the default num_beams is 3)
    with pytest.raises(ValueError, match="num_beams"):
        t.infer_requests([req], num_beams=3, timestamps=True, alignment_heads=HEADS)
    with pytest.raises(ValueError, match="timestamps"):
        t.infer_requests([req], num_beams=1, alignment_heads=HEADS)
    for bad in ([(3, 0)], [(0, 2)], [(-1, 0)], [(0, 0), (0, 0)], [], [(0, 0)] * 9, [0, 1], "x", [(l, h) for l in range(3) for h in range(2)] * 2):
        with pytest.raises(ValueError, match="alignment_heads"):
            t.infer_requests([req], num_beams=1, timestamps=True, alignment_heads=bad)
    with pytest.raises(ValueError, match="timestamps"):
        next(iter(t.infer_stream("a.wav", ["hello"], "en", timestamps=True)))
    with pytest.raises(ValueError, match="timestamps"):
        t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global", alignment_heads=HEADS)
    assert not t.gpt.calls and not t.frontend.calls                                 # every refusal came before any work
    # the engine's Python entries: no handle is touched (the objects have none)
    m = object.__new__(gpt.UnifiedVoice)
    m._loaded, m.layers, m.heads = True, 3, 2
    x, mask = torch.zeros(2, 4, 8), torch.ones(2, 5)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(x, mask, 8, num_beams=3, alignment_heads=HEADS, text_spans=[(0, 2), (0, 2)])
    with pytest.raises(ValueError, match="alignment_heads"):
        m.generate(x, mask, 8, alignment_heads=[(3, 0)], text_spans=[(0, 2), (0, 2)])
    with pytest.raises(ValueError, match="text_spans"):
        m.generate(x, mask, 8, alignment_heads=HEADS)
    with pytest.raises(ValueError, match="text_spans"):
        m.generate(x, mask, 8, alignment_heads=HEADS, text_spans=[(0, 2)])
    with pytest.raises(ValueError, match="text_spans"):
        m.generate(x, mask, 8, alignment_heads=HEADS, text_spans=[(0, 2), (0, 1025)])
    with pytest.raises(ValueError, match="text_spans"):
        m.generate(x, mask, 8, alignment_heads=HEADS, text_spans=[(0, 2), (12289, 4)])
    with pytest.raises(ValueError, match="text_spans"):
        m.generate(x, mask, 8, text_spans=[(0, 2), (0, 2)])
    with pytest.raises(ValueError, match="alignment_heads"):
        next(m.generate_chunks(x, mask, 8, 4, 1, num_beams=3, alignment_heads=HEADS, text_spans=[(0, 2), (0, 2)]))
    with pytest.raises(ValueError, match="alignment_heads"):
        gpt.BeamDecodeSession(m, x, mask, 8, num_beams=3, alignment_heads=HEADS)
    # `timestamps` is the v2.5 pipeline's kwarg: the engine entries (which the v2 and v1 pipelines forward their kwargs to) do not drop it silently
    with pytest.raises(ValueError, match="infer_requests"):
        m.generate(x, mask, 8, timestamps=True)
    with pytest.raises(ValueError, match="infer_requests"):
        next(m.generate_chunks(x, mask, 8, 4, 1, timestamps=True))
    with pytest.raises(ValueError, match="infer_requests"):
        gpt.DecodeSession._check_kwargs(None, dict(timestamps=True))


def test_unit_case_matrix_covers_what_it_claims():
    wins, pads, kinds = set(), set(), set()
    for c in R.CASES:
        for b, (pb, first, last, u, rstep, off, ln) in enumerate(R.geometry(c)):
            assert 0 <= first <= last < c.Tmax and 0 <= pb < R.ROWS and 0 <= u < R.UTTS
            assert (0 <= rstep < R.MAX_NEW) or not c.expect[b]
            n = last - first + 1
            pads.add(first)
            if c.expect[b] and ln > 0:                       # a window counts only where its row is written and compared
                wins.add((c.prec, n))
            if c.expect[b]:
                kinds.add("empty" if ln == 0 else "full" if ln == c.cap else "past" if off + ln > n else "tail" if off + ln == n else
                          "head" if (off, ln) == (0, 1) else "mid")
                kinds.add("odd") if ln % 4 else None
    for prec in (0, 1):
        assert {n for p, n in wins if p == prec} >= set(R.WINDOWS)
    assert pads >= set(R.PADS) and kinds >= {"empty", "full", "past", "tail", "head", "mid", "odd"}
    assert any(c.pos >= c.Tmax for c in R.CASES) and any(c.cap == 1024 for c in R.CASES)
    for name in ("shift", "seq_map", "row_slot", "row_step0"):
        assert {getattr(c, name) is None for c in R.CASES} == {True, False}, name
    assert {c.heads for c in R.CASES} == set(R.HEAD_SETS)
    assert any(not all(c.expect) for c in R.CASES)
    for c in R.CASES:                                        # where rows are skipped, a surviving row has keys to compare
        if not all(c.expect):
            assert any(e and g[6] > 0 for e, g in zip(c.expect, R.geometry(c))), c.name
    # the reference is a distribution over the window, and the bound is small against it
    c = next(c for c in R.CASES if c.name == "win-64-65-127" and c.prec == 1)
    q, k = R.operands(c)
    for u, rstep, ref, lim in R.reference(c, q, k):
        assert bool((ref >= 0).all()) and float(ref.sum(1).max()) <= 1 + 1e-12 and float(lim.max()) < 1e-4
    assert bool(torch.isnan(k).any())
