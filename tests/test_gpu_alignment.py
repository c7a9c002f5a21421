"""The text-attention export end to end (`generate(..., alignment_heads=, text_spans=)`, `itts_gpt_set_alignment`) on the tiny synthetic model
of the token-score tests (3 layers, 2 heads, three texts of 10 / 7 / 4 tokens, so three different left paddings), and the timestamps
`IndexTTS2.infer_requests(timestamps=True)` derives from it.

Exact (f32 bits, fp32 and bf16 engines): the export leaves the ids (and the token scores) alone; a row has, alone, the bits it has in a
9-row batch (past the 8-row fused-LayerNorm bucket), with and without compaction, through `generate_chunks`, and admitted into a
`DecodeSession` at a later step; row 0, forced columns and columns past the span are zero.
Against tests/align_ref.py (fp32 engine): the engine's own ids are teacher-forced through an f64 restatement of the GPT-2 stack, and the
exported rows are held to its softmax weights over the span."""
import os

import numpy as np
import pytest
import torch

from tests import align_ref as R
from tests.test_gpu_row_sampling import MAX_NEW, SEED, SETS
from tests.test_gpu_token_scores import _setup as _scores_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [(2, 0), (0, 1), (1, 0), (1, 1)]      # two layers, both heads of one layer, not in layer order
N = 9
CAPS = [MAX_NEW, 7, 25, 17, 12, MAX_NEW, 9, 30, 21]
# The restatement gate (test_rows_equal_the_f64_restatement): 4 x the largest |engine - f64 restatement| observed on the MI355X over the
# test's cases (GATE_OBSERVED); the margin is for other seeds, the fp32 engine is deterministic.  Above 1e-4 it would be a
# finding to explain, not a tolerance (the token-score test holds log-probabilities to 1.34e-5 through the same stack).
GATE_OBSERVED = 4.304e-8
GATE = 4 * GATE_OBSERVED
assert GATE <= 1e-4

_CACHE = {}


def _setup(golden_dir, prec):
    if prec in _CACHE:
        return _CACHE[prec]
    m, _, cfg, sd, _, _, style, emo, _ = _scores_setup(golden_dir, prec)
    z = np.load(os.path.join(golden_dir, "gpt_greedy.npz"))
    idx = [i % 3 for i in range(N)]
    text, langs = torch.from_numpy(z["text"])[idx].contiguous(), torch.from_numpy(z["langs"])[idx].contiguous()
    table = [dict(SETS[i % 4], seed=SEED + i, stream=0) for i in range(N)]

    def call(rows, **kw):
        """-> (ids on the host, the call's TokenAlignment with a host array or None)"""
        rows = list(rows)
        ids = m.inference_speech(None, text[rows], langs=langs[rows], emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW,
                                 num_beams=1, **kw)[0].cpu()
        al = m.last_alignment
        if al is not None:
            al = type(al)(al.attn.cpu(), al.text_lens, al.lengths)
        return ids, al

    def mixed(rows, **kw):
        rows = list(rows)
        return call(rows, row_sampling=[table[i] for i in rows], do_sample=False, seed=SEED, row_max_new=[CAPS[i] for i in rows], **kw)
    _CACHE[prec] = (m, call, mixed, cfg, sd, text, langs, style, emo, table)
    return _CACHE[prec]


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check_structure(ids, al, stop, caps):
    B, n = ids.shape
    assert al.attn.shape[:3] == (B, n, len(PAIRS)) and al.attn.dtype == torch.float32
    for b in range(B):
        L, T = int(al.lengths[b]), int(al.text_lens[b])
        hit = (ids[b] == stop).nonzero()
        first = int(hit[0]) if hit.numel() else n
        assert L == (first + 1 if first < caps[b] else caps[b]), (b, L, first, caps[b])
        a = al.attn[b].double()
        assert bool((a >= 0).all()) and bool(torch.isfinite(a).all())
        assert bool((a[0] == 0).all()), f"row {b}: code 0 comes from the prefill, its row must be zero"
        assert bool((a[L:] == 0).all()), f"row {b}: a forced column holds attention"
        assert bool((a[:, :, T:] == 0).all()), f"row {b}: columns past the span hold {a[:, :, T:].abs().max()}"
        s = a[1:L, :, :T].sum(-1)
        assert float(s.max() if s.numel() else 0.0) <= 1 + 1e-6
        if L > 1:
            assert bool((s > 0).all()), f"row {b}: a written row without any mass on the text"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_export_leaves_ids_and_scores_alone(golden_dir, prec):
    m, call, mixed, *_ = _setup(golden_dir, prec)
    rows = [0, 1, 2, 3]
    for s in (SETS[0], SETS[2]):                       # greedy, seeded sampling
        kw = {k: v for k, v in s.items()}
        off, none = call(rows, seed=SEED, **kw)
        assert none is None, "a call without heads leaves last_alignment = None"
        on, al = call(rows, seed=SEED, alignment_heads=PAIRS, **kw)
        assert torch.equal(on, off), "the ids changed with alignment_heads"
        _check_structure(on, al, m.stop_mel_token, [MAX_NEW] * 4)
        again, al2 = call(rows, seed=SEED, alignment_heads=PAIRS, **kw)
        assert torch.equal(again, off) and _bits(al.attn, al2.attn), "the same call twice"
        _, _ = call(rows, seed=SEED, token_scores=True, **kw)
        ts0 = m.last_scores
        both, al3 = call(rows, seed=SEED, token_scores=True, alignment_heads=PAIRS, **kw)
        ts1 = m.last_scores
        assert torch.equal(both, off) and _bits(al3.attn, al.attn)
        assert _bits(ts0.logp_model.cpu(), ts1.logp_model.cpu()) and _bits(ts0.logp_sampled.cpu(), ts1.logp_sampled.cpu())
    assert m.graph_stats() is not None


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("compaction", [False, True])
def test_a_row_alone_has_the_bits_it_has_in_the_nine_row_batch(golden_dir, prec, compaction):
    m, call, mixed, *_ = _setup(golden_dir, prec)
    key = ("alone", prec)
    if key not in _CACHE:
        _CACHE[key] = [mixed([i], alignment_heads=PAIRS) for i in range(N)]
    alone = _CACHE[key]
    m.set_compaction(compaction, 1)
    try:
        ids, al = mixed(range(N), alignment_heads=PAIRS)
        stats = dict(m.last_timing)
    finally:
        m.set_compaction(True, 8)
    assert stats["compactions"] >= 1 if compaction else stats["compactions"] == 0
    _check_structure(ids, al, m.stop_mel_token, CAPS)
    assert len(set(al.text_lens.tolist())) == 3
    for i in range(N):
        ids1, al1 = alone[i]
        L, T = int(al1.lengths[0]), int(al1.text_lens[0])
        assert int(al.lengths[i]) == L and int(al.text_lens[i]) == T and torch.equal(ids[i, :L], ids1[0, :L]), f"row {i}"
        assert _bits(al.attn[i, :L, :, :T], al1.attn[0, :L, :, :T]), f"row {i}: the export differs from the row alone"
    print(f"{prec} compaction={compaction}: lengths {al.lengths.tolist()} compactions {stats['compactions']}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_generate_chunks_and_admitted_rows_have_the_rows_own_bits(golden_dir, prec):
    from indextts_amd import gpt
    m, call, mixed, cfg, sd, text, langs, style, emo, table = _setup(golden_dir, prec)
    rows = [0, 1, 2, 3]
    ids, al = mixed(rows, alignment_heads=PAIRS)
    emb, mask, mn, hf = m.inference_speech_stream(None, text[rows], langs=langs[rows], emo_vec=emo, campplus_embedding=style,
                                                  max_generate_length=MAX_NEW, do_sample=False, num_beams=1, seed=SEED, alignment_heads=PAIRS)
    spans = hf["text_spans"]
    assert [l for _, l in spans] == al.text_lens.tolist() and all(o == 3 for o, _ in spans)          # 3 conditioning tokens, [start][ids][stop]
    # ---- generate_chunks (no caps there: compare with an uncapped call) ----
    ids_u, al_u = call(rows, row_sampling=[table[i] for i in rows], do_sample=False, seed=SEED, alignment_heads=PAIRS)
    kw = dict(hf)
    kw.pop("uniforms", None)
    for _ in m.generate_chunks(emb, mask, mn, 8, 2, row_sampling=[table[i] for i in rows], **kw):
        pass
    ch = m.last_alignment
    n = min(ch.attn.shape[1], al_u.attn.shape[1])
    for b in range(4):
        L = min(int(al_u.lengths[b]), n)
        assert _bits(ch.attn[b, :L].cpu(), al_u.attn[b, :L]), f"generate_chunks row {b}"
    assert sum(min(int(v), n) >= 8 for v in al_u.lengths) >= 2, "rows that run past the first chunk must exist, or the comparison shows nothing"
    # ---- a row admitted into a session at step 8, into the slot of a longer previous occupant ----
    new, new_cap = 5, 5                                     # utterance 5 (the shortest text) joins, capped below the slot's first occupant
    ids1, solo = call([new], row_sampling=[table[new]], do_sample=False, seed=SEED, row_max_new=[new_cap], alignment_heads=PAIRS)
    L, T = int(solo.lengths[0]), int(solo.text_lens[0])
    e1, m1, _, hf1 = m.inference_speech_stream(None, text[[new]], langs=langs[[new]], emo_vec=emo, campplus_embedding=style,
                                               max_generate_length=MAX_NEW, do_sample=False, num_beams=1, seed=SEED, alignment_heads=PAIRS)
    kw.pop("text_spans")
    caps = [MAX_NEW, 7, 25, 17]
    with gpt.DecodeSession(m, emb, mask, mn, row_sampling=[table[i] for i in rows], row_max_new=caps, text_spans=spans, **kw) as s:
        s.run(8)
        assert s.steps == 8 and 1 in s.finished()
        first = s.alignment(1)
        L0 = int(first.lengths[0])
        assert L0 == int(al.lengths[1]) > L and int(al.text_lens[1]) > T, "the previous occupant must be longer, or stale entries could not show"
        assert _bits(first.attn[0, :L0, :, :int(al.text_lens[1])].cpu(), al.attn[1, :L0, :, :int(al.text_lens[1])])
        with pytest.raises(ValueError, match="text_spans"):
            s.admit([1], e1, m1, row_max_new=[new_cap], row_sampling=[table[new]])
        s.admit([1], e1, m1, row_max_new=[new_cap], row_sampling=[table[new]], text_spans=hf1["text_spans"])
        while 1 not in s.finished() and s.steps < 8 + 2 * MAX_NEW:
            s.run(8)
        got = s.alignment(1)
        assert int(got.lengths[0]) == L and int(got.text_lens[0]) == T
        assert torch.equal(s._codes[1, :L].cpu(), ids1[0, :L])
        assert _bits(got.attn[0, :L, :, :T].cpu(), solo.attn[0, :L, :, :T]), "admitted at step 8: the export differs from the row alone"
        assert bool((s._al[1][1, L:] == 0).all()) and bool((s._al[1][1, :, :, T:] == 0).all()), "stale attention of the previous occupant"
        assert bool((s._al[1][1, 0] == 0).all())
    print(f"{prec}: admitted row: {L} codes over {T} text positions")


@pytest.mark.parametrize("si", [0, 2])
def test_rows_equal_the_f64_restatement(golden_dir, si):
    m, call, mixed, cfg, sd, text, langs, style, emo, table = _setup(golden_dir, "fp32")
    rows = [0, 1, 2]
    ids, al = call(rows, seed=SEED, alignment_heads=PAIRS, min_new_tokens=8, **SETS[si])       # (the first text's row would stop at once)
    emb, mask, mn, hf = m.inference_speech_stream(None, text[rows], langs=langs[rows], emo_vec=emo, campplus_embedding=style,
                                                  max_generate_length=MAX_NEW, num_beams=1, alignment_heads=PAIRS)
    x, pad, S = m._prefix(emb, mask)
    worst, count = 0.0, 0
    for b in rows:
        L, T = int(al.lengths[b]), int(al.text_lens[b])
        assert L >= 4
        want = R.teacher_forced_alignment(sd, cfg.layers, cfg.heads, x[b].cpu(), int(pad[b]), ids[b, :L].tolist(), PAIRS, hf["text_spans"][b])
        err = (al.attn[b, :L, :, :T].double() - want).abs()
        worst, count = max(worst, float(err.max())), count + err[1:].numel()
        assert float(want[1:].sum(-1).min()) > 1e-3, "the span must carry attention mass, or the comparison shows nothing"
        # the pairs are different numbers: an export that wrote one head to every pair must fail
        assert float((want[1:, 0] - want[1:, 1]).abs().max()) > 10 * GATE and float((want[1:, 2] - want[1:, 3]).abs().max()) > 10 * GATE
    print(f"set {si}: {count} exported weights, max |engine - f64 restatement| = {worst:.3e} (gate {GATE:.3e})")
    assert worst <= GATE


# ---- the pipeline's timestamps ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tts():
    from tests.test_gpu_mixed_requests import VoiceFrontend
    from tests.test_gpu_pipeline import build
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    return t


REQS = [dict(spk_audio_prompt="alice.wav", text="hello world", lang="en", seed=11),
        dict(spk_audio_prompt="bob.wav", text="a much longer second sentence here. ok", lang="en", seed=12, temperature=1.1, duration_factor=1.25),
        dict(spk_audio_prompt="carol.wav", text="one more for the first voice", lang="en", seed=13, top_k=8)]


@pytest.mark.filterwarnings("ignore:WARN. generation stopped:RuntimeWarning")
def test_timestamps_cover_the_waveform_and_do_not_depend_on_batch_mates(tts):
    kw = dict(num_beams=1, max_mel_tokens=24, timestamps=True, alignment_heads=[(1, 0), (0, 1)], interval_silence=100)
    outs = tts.infer_requests(REQS, **kw)
    ts = tts.last_timestamps
    assert len(ts) == 3 and [len(t) for t in ts] == [1, 2, 1]
    sil = int(22050 * 0.1)
    for r, (sr, w) in enumerate(outs):
        flat = [e for seg in ts[r] for e in seg]
        assert flat and all(e["start"] <= e["end"] for e in flat)
        assert all(a["end"] <= b["start"] + 1e-12 for a, b in zip(flat, flat[1:])), f"request {r}: timestamps decrease"
        assert ts[r][0][0]["start"] == 0.0 and abs(flat[-1]["end"] - w.shape[0] / 22050.0) < 1e-9, "the entries cover the waveform"
        for a, b in zip(ts[r], ts[r][1:]):                 # a segment starts one silence after the previous one ends
            assert abs(b[0]["start"] - a[-1]["end"] - sil / 22050.0) < 1e-9
        assert all(isinstance(e["text_id"], int) for e in flat)
    assert ts[1][0][-1]["end"] > ts[1][0][0]["start"]
    # alone, in another order, and through the in-flight scheduler
    for r in range(3):
        tts.infer_requests([REQS[r]], **kw)
        assert tts.last_timestamps == [ts[r]], f"request {r} alone"
    tts.infer_requests(REQS[::-1], **kw)
    assert tts.last_timestamps == ts[::-1]
    tts.infer_requests(REQS, inflight_slots=2, chunk_tokens=4, **kw)
    assert tts.last_timestamps == ts
    with pytest.raises(ValueError, match="alignment_heads"):
        tts.infer_requests(REQS, num_beams=1, timestamps=True)
    tts.alignment_heads = [(1, 0), (0, 1)]
    try:
        tts.infer_requests(REQS, **{k: v for k, v in kw.items() if k != "alignment_heads"})
        assert tts.last_timestamps == ts
    finally:
        tts.alignment_heads = None


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_another_pair_list_never_replays_the_previous_step_graph(golden_dir, prec):
    """the same shapes, so the same persistent span / output buffers: only the install epoch of the graph key tells the two calls apart"""
    m, call, mixed, *_ = _setup(golden_dir, prec)
    rows = [1, 2, 4, 5]
    ids, al = mixed(rows, alignment_heads=PAIRS)
    ids_r, al_r = mixed(rows, alignment_heads=PAIRS[::-1])
    ids_2, al_2 = mixed(rows, alignment_heads=PAIRS[:2] + [(0, 0), (2, 1)])
    assert torch.equal(ids, ids_r) and torch.equal(ids, ids_2)
    K = len(PAIRS)
    for k in range(K):
        assert _bits(al_r.attn[:, :, k], al.attn[:, :, K - 1 - k]), f"pair {k} of the reversed list"
    assert _bits(al_2.attn[:, :, :2], al.attn[:, :, :2]) and not _bits(al_2.attn[:, :, 2:], al.attn[:, :, 2:])
    off, none = mixed(rows)
    assert none is None and torch.equal(off, ids)


def test_engine_refuses_other_shapes_and_beams_while_an_export_is_installed(golden_dir):
    from indextts_amd import _lib
    m, call, mixed, cfg, sd, text, langs, style, emo, table = _setup(golden_dir, "fp32")
    two = lambda **kw: m.inference_speech(None, text[[0, 1]], langs=langs[[0, 1]], emo_vec=emo, campplus_embedding=style, do_sample=False, **kw)
    m._install_alignment(([(0, 0)], [(3, 4), (3, 4)]), 2, MAX_NEW)          # serves calls of exactly 2 utterances and MAX_NEW tokens
    try:
        with pytest.raises(_lib.HipEngineError, match="itts_gpt_set_alignment"):
            call([0, 1, 2], seed=SEED, do_sample=False)                       # another utterance count
        with pytest.raises(_lib.HipEngineError, match="itts_gpt_set_alignment"):
            two(max_generate_length=MAX_NEW - 1, num_beams=1)                 # another max_new_tokens
        with pytest.raises(_lib.HipEngineError, match="num_beams = 1 only"):
            two(max_generate_length=MAX_NEW, num_beams=3)                     # a beam call
    finally:
        m._uninstall_alignment()
    L = _lib.lib()
    sp, out = torch.zeros(2, 2, dtype=torch.int32, device=DEV), torch.zeros(2 * MAX_NEW * 8, device=DEV)
    import ctypes as C
    arr = lambda *v: (C.c_int32 * len(v))(*v)
    bad = [(arr(3, 0), 1, 8), (arr(0, 2), 1, 8), (arr(0, 0, 0, 0), 2, 8), (arr(0, 0), 1, 6), (arr(0, 0), 1, 1028), (arr(0, 0), 0, 8), (arr(*([0, 0] * 9)), 9, 8)]
    for pairs, n_pairs, cap in bad:
        assert L.itts_gpt_set_alignment(m._h, pairs, n_pairs, _lib.ptr(sp), _lib.ptr(out), 2, MAX_NEW, cap) == _lib.ERR_ARG, (list(pairs), n_pairs, cap)
    ids, al = call([0, 1], seed=SEED, do_sample=False)                        # nothing stayed installed
    assert al is None
