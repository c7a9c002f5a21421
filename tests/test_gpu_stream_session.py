"""`IndexTTS2.stream_session` on the real HIP engines (tiny random models, the engine's codec and s2mel stages in fp32, a per-voice stub front
end): a stream's events -- int16 pieces, done flags, chunk indices -- are bit for bit those of `infer_stream` over the request alone, whatever
slot it got, whatever step it joined at, whatever its batch mates are; a session opened by a short request admits the longest prompt; a
cancelled stream's slot is reused; and `close()` gives the engine back."""
import numpy as np
import pytest
import torch

from tests.test_gpu_cfm_noise_pipeline import VoiceFrontend
from tests.test_gpu_pipeline import _s2_engines, build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK, OVERLAP = 8, 2
STRIDE = CHUNK - OVERLAP
MAX_TEXT = 30                                            # max_text_tokens_per_segment of the sessions and of the alone runs
SESSION = dict(chunk_size=CHUNK, overlap_size=OVERLAP, max_mel_tokens=24, max_text_tokens_per_segment=MAX_TEXT)

# caps: below one chunk (5), on a chunk boundary (14 = 8 + 6, 20 = 8 + 2 * 6), off a boundary (24, 17)
REQUESTS = [
    dict(spk_audio_prompt="alice.wav", text="hello world", lang="en", seed=11, max_mel_tokens=5),
    dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=12, max_mel_tokens=14, temperature=1.1, top_k=12),
    dict(spk_audio_prompt="carol.wav", text="a much longer second sentence", lang="en", seed=13, max_mel_tokens=20),
    dict(spk_audio_prompt="alice.wav", text="one more for the first voice", lang="en", seed=14, max_mel_tokens=24, duration_factor=1.25),
    dict(spk_audio_prompt="bob.wav", text="and the last one", lang="en", seed=15, max_mel_tokens=17),
]
LONG = dict(spk_audio_prompt="carol.wav", text="this text has more characters than a segment may hold tokens", lang="en", seed=21,
            max_mel_tokens=16)
SHORT = dict(spk_audio_prompt="bob.wav", text="ok", lang="en", seed=22, max_mel_tokens=11)
DETERMINISM = dict(max_mel_tokens=24, chunk_size=8, overlap_size=2, seed=9, cfm_noise="request")      # the call of the infer_stream determinism test


def run_alone(tts, req):
    """[(piece, done, chunk index)] of row 0 of infer_stream over the request alone"""
    r = dict(req)
    gen = tts.infer_stream(r.pop("spk_audio_prompt"), [r.pop("text")], r.pop("lang"), chunk_size=CHUNK, overlap_size=OVERLAP,
                           max_text_tokens_per_segment=MAX_TEXT, cfm_noise="request", **r)
    return [(audio[0], bool(done[0]), k) for k, (_, audio, done) in enumerate(gen)]


def determinism_call(tts):
    return [(audio, list(done)) for _, audio, done in tts.infer_stream("spk.wav", ["a first streamed sentence", "short"], "en", **DETERMINISM)]


@pytest.fixture(scope="module")
def tts():
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    t.semantic_codec, t.s2mel = _s2_engines("fp32")[:2]
    return t


@pytest.fixture(scope="module")
def alone(tts):
    """every request alone, once; and the determinism test's call before any session ran"""
    ref = [run_alone(tts, r) for r in REQUESTS]
    for r, ev in zip(REQUESTS, ref):
        print(f"alone: cap {r['max_mel_tokens']}: {len(ev)} events, {sum(len(p) for p, _, _ in ev if p is not None)} samples")
        assert ev and ev[-1][1] and np.abs(np.concatenate([p for p, _, _ in ev])).max() > 0
    return ref, determinism_call(tts)


def drain(sess, submit_late=(), cancel=None):
    """{stream id: [(piece, done, chunk index)]}; submit_late: [(number of step() calls before, request)]; cancel: (stream id, steps before)"""
    out, ids, n = {}, [], 0
    late = list(submit_late)
    while sess.active or late:
        for item in [x for x in late if x[0] <= n]:
            ids.append(sess.submit(item[1]))
            late.remove(item)
        if cancel is not None and cancel[1] == n:
            assert sess.cancel(cancel[0])
        for sid, sr, piece, done, k in sess.step():
            assert sr == 22050
            out.setdefault(sid, []).append((piece, done, k))
        n += 1
        assert n < 400
    return out, ids


def same_events(got, ref, what):
    assert [(d, k) for _, d, k in got] == [(d, k) for _, d, k in ref], what
    for (p, _, k), (p0, _, _) in zip(got, ref):
        assert p is not None and p.dtype == np.int16 and p.shape == p0.shape, f"{what}: chunk {k}: {p.shape} vs {p0.shape}"
        assert np.array_equal(p, p0), f"{what}: chunk {k}: max|d| {int(np.abs(p.astype(np.int32) - p0.astype(np.int32)).max())}"


@pytest.mark.parametrize("slots", [2, 3])
def test_streams_are_bit_equal_to_the_request_alone(tts, alone, slots):
    ref, _ = alone
    torch.manual_seed(1)
    with tts.stream_session(slots=slots, **SESSION) as sess:
        ids = [sess.submit(r) for r in REQUESTS]
        torch.randn(5, device=DEV)                               # whatever torch's generator holds
        out, _ = drain(sess)
        stats = sess.stats
    for i, sid in enumerate(ids):
        same_events(out[sid], ref[i], f"slots {slots}: request {i}")
    joined = [stats["streams"][sid]["admitted_step"] for sid in ids]
    print(f"slots {slots}: admitted at session steps {joined}, slots {[stats['streams'][s]['slot'] for s in ids]}, rows per render "
          f"{stats['render_rows']}")
    assert joined[:slots] == [0] * slots and all(s > 0 for s in joined[slots:])
    assert any(s % STRIDE != 0 for s in joined)                   # a stream joined off the chunk grid of its batch mates
    assert max(stats["render_rows"]) > 1 and all(stats["streams"][sid]["first_audio_s"] > 0 for sid in ids)


def test_order_and_slot_independence(tts, alone):
    ref, _ = alone
    rev = REQUESTS[::-1]
    with tts.stream_session(slots=2, poll_steps=3, **SESSION) as sess:
        ids = [sess.submit(r) for r in rev[:-1]]
        out, late_ids = drain(sess, submit_late=[(2, rev[-1])])   # REQUESTS[0] arrives after two step() calls
    for sid, i in zip(ids + late_ids, range(len(REQUESTS) - 1, -1, -1)):
        same_events(out[sid], ref[i], f"reversed: request {i}")


def test_a_session_opened_by_a_short_request_admits_the_longest_prompt(tts):
    # the stub tokenises a character per token and cuts at the segment limit: MAX_TEXT tokens and the stop id
    assert tts.frontend.text_segments(LONG["text"], "en", MAX_TEXT, True, 0)[0].numel() == MAX_TEXT + 1
    ref_long, ref_short = run_alone(tts, LONG), run_alone(tts, SHORT)
    with tts.stream_session(slots=2, **SESSION) as sess:          # one stream on two slots: the other starts empty
        first = sess.submit(SHORT)
        out, (second,) = drain(sess, submit_late=[(1, LONG)])     # the long one arrives after the session was opened
        stats = sess.stats
    same_events(out[first], ref_short, "the short opener")
    same_events(out[second], ref_long, "the long prompt")
    assert stats["streams"][first]["admitted_step"] == 0 and stats["streams"][second]["admitted_step"] > 0


def test_cancel_mid_stream_frees_the_slot(tts, alone):
    ref, _ = alone
    samples = [sum(len(p) for p, _, _ in ev) for ev in ref]
    order = sorted(range(len(REQUESTS)), key=lambda i: -samples[i])          # the two longest open the session, the longest is cancelled
    with tts.stream_session(slots=2, **SESSION) as sess:
        ids = [sess.submit(REQUESTS[i]) for i in order]
        out, _ = drain(sess, cancel=(ids[0], 1))                  # after one poll
        stats = sess.stats
    gone = out[ids[0]]
    assert [d for _, d, _ in gone] == [False] * (len(gone) - 1) + [True] and gone[-1][0] is None and len(gone) <= len(ref[order[0]])
    same_events(gone[:-1], ref[order[0]][:len(gone) - 1], "the cancelled stream before its cancel")
    for sid, i in zip(ids[1:], order[1:]):
        same_events(out[sid], ref[i], f"after a cancel: request {i}")
    slot = stats["streams"][ids[0]]["slot"]
    reused = [sid for sid in ids[2:] if stats["streams"][sid]["slot"] == slot]
    print(f"cancelled in slot {slot} after {len(gone) - 1} pieces; then served there: {reused}")
    assert reused                                                 # a waiting request took the cancelled slot


def test_close_releases_the_engine(tts, alone):
    _, before = alone
    sess = tts.stream_session(slots=2, **SESSION)
    sess.submit(REQUESTS[2])
    assert sess.step() is not None
    with pytest.raises(RuntimeError, match="is open on this engine"):
        tts.infer_batch("alice.wav", ["hello world"], "en", num_beams=1, max_mel_tokens=8)
    sess.close()
    sr, wav = tts.infer_batch("alice.wav", ["hello world"], "en", num_beams=1, max_mel_tokens=8, seed=3)[0]
    assert sr == 22050 and wav.shape[0] > 0
    after = determinism_call(tts)
    assert len(after) == len(before) >= 2
    for (a0, d0), (a1, d1) in zip(before, after):
        assert d0 == d1
        for x, y in zip(a0, a1):
            assert (x is None) == (y is None) and (x is None or np.array_equal(x, y))
