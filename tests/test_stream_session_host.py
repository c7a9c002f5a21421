"""CPU tests of the streaming session's host side (`streaming.StreamSession`, `streaming.RowStream`, `serving.StreamBatcher`) over a scripted
fake decode session -- every row's codes are given in advance -- and a deterministic fake renderer whose samples depend on the window's codes,
the chunk index and the stream's seed: the per-stream chunker against `StreamingDecoder` over the chunk loop of `generate_chunks` for B = 1,
the scheduling rules, `cancel`, the errors, and the thread-safe batcher."""
import threading

import numpy as np
import pytest

from indextts_amd import streaming

STOP = 8193
CHUNK, OVERLAP = 8, 2
STRIDE = CHUNK - OVERLAP
FPC = 2.0                                                # mel frames per code of the fake renderer: 512 samples per code


def fake_audio(codes, k, seed):
    """float32 samples of a window: 512 per code, a function of the code, the chunk index and the seed"""
    ramp = np.linspace(0.0, 0.2, 512, dtype=np.float32)
    parts = [((int(c) % 97) / 200.0 + 0.01 * k + 0.001 * (seed % 50)) - ramp for c in codes]
    return np.concatenate(parts).astype(np.float32) if parts else np.zeros(0, dtype=np.float32)


def script(n, seed):
    """n + 40 codes, none of them the stop token"""
    rng = np.random.default_rng(seed)
    return [int(v) for v in rng.integers(0, 8000, n + 40)]


# ---- the reference side: the chunk loop of UnifiedVoice._generate_chunks_body for one scripted row + StreamingDecoder ---------------
class ScriptedEngine:
    """`generate_chunks` for B = 1 over a scripted row: the row's token at index i is codes[i], the stop token from index `stop_at` on (None:
    never); the loop, its limits and what it yields are those of `_generate_chunks_body`."""

    def __init__(self, codes, stop_at):
        self.codes, self.stop_at = codes, stop_at

    def token(self, i):
        return STOP if self.stop_at is not None and i >= self.stop_at else self.codes[i]

    def generate_chunks(self, inputs_embeds, attention_mask, max_new, chunk_size, overlap_size, **kw):
        stride = chunk_size - overlap_size
        steps, next_chunk_at, buf = 0, chunk_size, []
        while True:
            limit = min(next_chunk_at, max_new)
            while steps < limit:                         # the engine returns at the limit, or when every row has emitted its stop token
                buf.append(self.token(steps))
                steps += 1
                if buf[-1] == STOP:
                    break
            done = STOP in buf
            n = buf.index(STOP) if done else steps
            finished = done or steps >= max_new or steps < limit
            while n >= next_chunk_at:
                pos = next_chunk_at - chunk_size
                yield np.asarray([buf[pos:next_chunk_at]]), False, [done and n <= next_chunk_at], np.asarray([max(0, min(n - pos, chunk_size))])
                next_chunk_at += stride
            if finished:
                pos = next_chunk_at - chunk_size
                if pos < n:
                    yield np.asarray([buf[pos:n]]), True, [True], np.asarray([max(0, n - pos)])
                return


def alone(codes, n, ended_by, seed):
    """[(int16 piece, done, chunk index)] of the row alone: n codes, ended by its own stop token or by its cap"""
    eng = ScriptedEngine(codes, n if ended_by == "stop" else None)
    max_new = n + 25 if ended_by == "stop" else n
    dec = streaming.StreamingDecoder(eng, lambda c, lens: [fake_audio(c[0, : int(lens[0])], dec.chunk_index, seed)], chunk_size=CHUNK,
                                     overlap_size=OVERLAP, frames_per_code=FPC)
    out = []
    for k, (sr, audio, done) in enumerate(dec.generate(np.zeros((1, 1, 1)), None, max_new)):
        assert sr == 22050
        out.append((audio[0], bool(done[0]), k))
    return out


# ---- the session side: a scripted decode session behind the backend interface -------------------------------------------------------
class FakeBackend:
    """rows advance one token per step; an admitted row has its first token at once (the admission computes it); a row's token at index i is
    its script's, the stop token from its own stop index or its cap on -- the two look the same from here, as on the engine"""
    KEYS = {"codes", "n", "ended_by", "seed", "name"}

    def __init__(self, flag_every=4):
        self.steps, self.rows, self.step0 = 0, [], []
        self.flag_every = flag_every                     # with return_when_finished the engine looks at its flags every few steps
        self.admissions, self.renders, self.stopped, self.closed = [], [], [], False

    def prepare(self, req):
        unknown = sorted(set(req) - self.KEYS)
        if unknown:
            raise ValueError(f"unknown keys {unknown}")
        return dict(req, end=req["n"])

    def frames_per_code(self, item):
        return FPC

    def open(self, items):
        self.rows = [it if it is not None else dict(end=0, codes=[], name=None) for it in items]
        self.rows = [dict(r) for r in self.rows]
        self.step0 = [0] * len(items)
        self.admissions += [(0, s, it["name"]) for s, it in enumerate(items) if it is not None]

    def _own(self, slot):
        return self.steps - self.step0[slot]

    def _ended(self, slot):
        return self._own(slot) > self.rows[slot]["end"]       # the stop token at index `end` has been emitted

    def admit(self, slots, items):
        assert self.steps >= 1
        for s, it in zip(slots, items):
            assert self._ended(s), f"slot {s} admitted while its row is still generating"
            self.rows[s], self.step0[s] = dict(it), self.steps - 1
            self.admissions.append((self.steps, s, it["name"]))

    def run(self, n, return_when_finished):
        for _ in range(n):
            self.steps += 1
            if return_when_finished and self.steps % self.flag_every == 0 and \
                    sum(self._ended(s) for s in range(len(self.rows))) >= return_when_finished:
                break

    def progress(self):
        return [(max(0, min(self._own(s), self.rows[s]["end"])), self._ended(s)) for s in range(len(self.rows))]

    def stop(self, slot):
        self.rows[slot]["end"] = min(self.rows[slot]["end"], max(0, self._own(slot)))
        self.stopped.append(slot)

    def collect(self, jobs):
        return [list(self.rows[slot]["codes"][pos:pos + n]) for _, slot, _, pos, n in jobs]

    def render(self, jobs, windows):
        self.renders.append(len(jobs))
        return [fake_audio(w, k, item["seed"]) for (item, _, k, _, _), w in zip(jobs, windows)]

    def close(self):
        self.closed = True


def request(name, n, ended_by="stop", seed=None):
    seed = sum(map(ord, name)) if seed is None else seed
    return dict(name=name, n=n, ended_by=ended_by, seed=seed, codes=script(n, seed))


def run_session(reqs, slots, poll_steps, late=(), cancel=None):
    """-> ({name: [(piece, done, chunk index)]}, backend, session).  late: {index: number of step() calls before it is submitted};
    cancel: (name, number of step() calls before the cancel)"""
    late = dict(late)
    be = FakeBackend()
    sess = streaming.StreamSession(be, slots, chunk_size=CHUNK, overlap_size=OVERLAP, poll_steps=poll_steps)
    name_of, out = {}, {}
    for i, r in enumerate(reqs):
        if i not in late:
            name_of[sess.submit(r)] = r["name"]
    n_steps = 0
    while sess.active or any(v >= n_steps for v in late.values()):
        for i, at in list(late.items()):
            if at == n_steps:
                name_of[sess.submit(reqs[i])] = reqs[i]["name"]
                del late[i]
        if cancel is not None and cancel[1] == n_steps:
            assert sess.cancel([s for s, n in name_of.items() if n == cancel[0]][0])
        for sid, sr, piece, done, k in sess.step():
            assert sr == 22050
            out.setdefault(name_of[sid], []).append((piece, done, k))
        n_steps += 1
        assert n_steps < 500
    return out, be, sess


def same_events(a, b):
    assert len(a) == len(b), (len(a), len(b))
    for (p, d, k), (p0, d0, k0) in zip(a, b):
        assert (d, k) == (d0, k0)
        assert (p is None) == (p0 is None)
        if p is not None:
            assert p.dtype == np.int16 and np.array_equal(p, p0)


LENGTHS = [1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + STRIDE - 1, CHUNK + STRIDE, CHUNK + STRIDE + 1, CHUNK + 2 * STRIDE]


@pytest.mark.parametrize("ended_by", ["stop", "cap"])
@pytest.mark.parametrize("n", LENGTHS)
def test_chunker_matches_streaming_decoder_over_generate_chunks(n, ended_by):
    r = request(f"row{n}", n, ended_by)
    ref = alone(r["codes"], n, ended_by, r["seed"])
    assert ref and ref[-1][1] and not any(d for _, d, _ in ref[:-1])
    for poll in (1, 8, 13):
        out, be, _ = run_session([r], 1, poll)
        same_events(out[r["name"]], ref)
        assert len(out[r["name"]]) == len(ref)
    # in a batch, joining late: the same events
    mates = [request("m0", 11), request("m1", 3, "cap"), r, request("m2", 17)]
    out, _, sess = run_session(mates, 2, 5)
    same_events(out[r["name"]], ref)


def test_row_stream_windows():
    row = streaming.RowStream(CHUNK, OVERLAP, FPC)
    assert row.due(7, False) == [] and row.due(8, False) == [(0, 0, 8, False)] and row.due(13, False) == []
    assert row.due(21, False) == [(1, 6, 8, False), (2, 12, 8, False)]             # a long poll: two chunks at once
    assert row.due(21, True) == [(3, 18, 3, True)]
    short = streaming.RowStream(CHUNK, OVERLAP, FPC)
    assert short.due(0, True) == [] and short.flush() is None                      # a row without codes has nothing to say
    exact = streaming.RowStream(CHUNK, 0, FPC)                                     # no overlap, the row ends on a boundary: no closing chunk
    assert exact.due(8, True) == [(0, 0, 8, False)]
    exact.push(fake_audio(range(8), 0, 0), False)
    assert exact.flush().shape == (0,) and exact.finished


SEVEN = [("a", 20, "stop"), ("b", 5, "cap"), ("c", 14, "cap"), ("d", 9, "stop"), ("e", 1, "stop"), ("f", 26, "cap"), ("g", 13, "stop")]


@pytest.fixture(scope="module")
def seven_alone():
    reqs = [request(*r) for r in SEVEN]
    return reqs, {r["name"]: alone(r["codes"], r["n"], r["ended_by"], r["seed"]) for r in reqs}


@pytest.mark.parametrize("poll", [1, 8, 13])
def test_scheduling_seven_requests_on_three_slots(seven_alone, poll):
    reqs, ref = seven_alone
    out, be, sess = run_session(reqs, 3, poll)
    names = [r["name"] for r in reqs]
    assert [a[2] for a in be.admissions] == names                                  # every request once, in FIFO order (admit asserts the slot had ended)
    assert [a[0] for a in be.admissions[:3]] == [0, 0, 0] and all(a[0] >= 1 for a in be.admissions[3:])
    for name in names:
        ev = out[name]
        assert [k for _, _, k in ev] == list(range(len(ev)))                       # increasing chunk indices
        assert [d for _, d, _ in ev] == [False] * (len(ev) - 1) + [True]           # exactly one done, last
        same_events(ev, ref[name])                                                 # ... and identical whatever poll_steps is
    st = sess.stats
    assert sorted(st["streams"]) == list(range(7)) and st["render_rows"] == be.renders and sum(be.renders) == sum(len(ref[n]) for n in names)
    for sid, rec in st["streams"].items():
        assert (rec["admitted_step"], rec["slot"]) == be.admissions[sid][:2] and rec["first_audio_s"] >= 0.0
    assert max(be.renders) > 1                                                     # chunks of several rows share a render
    assert not sess.active


def test_fewer_streams_than_slots_and_a_late_submit(seven_alone):
    reqs, ref = seven_alone
    out, be, sess = run_session(reqs[:2] + [reqs[5]], 4, 8, late={2: 2})
    for r in reqs[:2] + [reqs[5]]:
        same_events(out[r["name"]], ref[r["name"]])
    assert be.admissions[2][0] >= 1 and be.admissions[2][2] == "f"
    # an idle session (every row ended) takes a new stream
    sid = sess.submit(reqs[3])
    ev = [(p, d, k) for s, _, p, d, k in sess.events() if s == sid]
    same_events(ev, ref["d"])


def test_cancel_live_and_waiting(seven_alone):
    reqs, ref = seven_alone
    out, be, sess = run_session(reqs, 3, 8, cancel=("a", 1))                       # "a" (20 codes) is live in slot 0 after one step
    assert be.stopped == [0]
    ev = out["a"]
    assert [d for _, d, _ in ev] == [False] * (len(ev) - 1) + [True] and ev[-1][0] is None and len(ev) < len(ref["a"]) + 1
    same_events(ev[:-1], ref["a"][:len(ev) - 1])                                   # what it had got before is what it gets alone
    for name in "bcdefg":
        same_events(out[name], ref[name])                                          # the others are unchanged
    cancelled_at = 8                                                               # the session step of the cancel (one poll of 8)
    refill = [a for a in be.admissions if a[1] == 0 and a[0] > 0][0]
    assert cancelled_at < refill[0] <= cancelled_at + 8                            # slot 0 is refilled at the next poll
    # a waiting request
    be2 = FakeBackend()
    s2 = streaming.StreamSession(be2, 1, chunk_size=CHUNK, overlap_size=OVERLAP, poll_steps=8)
    i0, i1, i2 = (s2.submit(r) for r in reqs[:3])
    assert s2.cancel(i1) and not s2.cancel(i1) and not s2.cancel(99)
    got = {}
    for sid, _, p, d, k in s2.events():
        got.setdefault(sid, []).append((p, d, k))
    assert len(got[i1]) == 1 and got[i1][0][0] is None and got[i1][0][1] is True
    same_events(got[i0], ref["a"])
    same_events(got[i2], ref["c"])
    assert [a[2] for a in be2.admissions] == ["a", "c"]
    s2.close()
    assert be2.closed


def test_session_errors():
    be = FakeBackend()
    sess = streaming.StreamSession(be, 2, chunk_size=CHUNK, overlap_size=OVERLAP)
    with pytest.raises(ValueError, match="unknown keys"):
        sess.submit(dict(request("x", 3), voice="v"))
    sess.close()
    with pytest.raises(RuntimeError, match="closed"):
        sess.submit(request("x", 3))
    with pytest.raises(ValueError):
        streaming.StreamSession(be, 2, chunk_size=8, overlap_size=8)
    with pytest.raises(ValueError):
        streaming.StreamSession(be, 0)


# ---- the pipeline's binding: validation without a GPU -------------------------------------------------------------------------------
def _cpu_tts():
    import torch
    from indextts_amd.infer_v2_5 import IndexTTS2
    from tests.pipeline_stubs import StubFrontend
    from tests.test_pipeline_cpu import FakeGPT, FakeVoc

    class Gpt(FakeGPT):
        def conds_latent(self, style, emo_vec):
            return torch.zeros(1, 3, 64), None

        @staticmethod
        def _seed(seed, do_sample, uniforms):
            return 7 if seed is None else int(seed)

    return IndexTTS2(cfg={"gpt": {"stop_mel_token": 8193}}, device="cpu", frontend=StubFrontend(64), gpt=Gpt(), bigvgan=FakeVoc())


def test_pipeline_session_checks_requests_like_infer_requests():
    tts = _cpu_tts()
    sess = tts.stream_session(slots=2, chunk_size=CHUNK, overlap_size=OVERLAP, max_mel_tokens=24, cfm_noise="global", top_k=5)
    with pytest.raises(ValueError, match="unknown keys"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", voice="x"))
    with pytest.raises(ValueError, match="unknown keys"):                          # the same refusal as the batch path
        tts.infer_requests([dict(spk_audio_prompt="a.wav", text="hello", lang="en", voice="x")], num_beams=1)
    with pytest.raises(ValueError, match="one segment"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="one. two", lang="en"))
    with pytest.raises(ValueError, match="max_mel_tokens"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", max_mel_tokens=25))
    with pytest.raises(ValueError, match="typical_mass"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", typical_sampling=True, typical_mass=1.5))
    sid = sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", temperature=1.1))
    item = sess._waiting[0][1]
    assert sid == 0 and item.entry["top_k"] == 5 and item.entry["temperature"] == 1.1 and item.entry["stream"] == 0
    assert item.seed == item.entry["seed"] == 7 and item.cap == 24                 # no seed given: drawn at submit
    assert sess.cancel(sid) and sess.step() == [(0, 22050, None, True, 0)]         # nothing was opened: no engine needed
    sess.close()
    with pytest.raises(RuntimeError, match="closed"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en"))
    with pytest.raises(ValueError, match="cfm_noise='request'"):                   # keyed noise needs the engine's codes -> mel stages
        tts.stream_session(slots=2)
    with pytest.raises(ValueError, match="cfm_noise"):
        tts.stream_session(slots=2, cfm_noise="other")


def test_other_pipelines_refuse():
    from indextts_amd.infer_v2 import IndexTTS2 as V2
    v2 = object.__new__(V2)
    with pytest.raises(NotImplementedError):
        v2.stream_session(slots=2)
    from indextts_amd.infer import IndexTTS
    with pytest.raises(NotImplementedError):
        object.__new__(IndexTTS).stream_session(slots=2)


# ---- StreamBatcher ------------------------------------------------------------------------------------------------------------------
class _FakeSessionTTS:
    def __init__(self):
        self.backend, self.kwargs = FakeBackend(), None

    def stream_session(self, slots, **kw):
        self.kwargs = dict(kw, slots=slots)
        return streaming.StreamSession(self.backend, slots, chunk_size=CHUNK, overlap_size=OVERLAP, poll_steps=kw.get("poll_steps", 8))


def test_stream_batcher_routes_pieces_to_their_iterators(seven_alone):
    from indextts_amd.serving import StreamBatcher
    reqs, ref = seven_alone
    tts = _FakeSessionTTS()
    b = StreamBatcher(tts, slots=2, poll_steps=5)
    assert tts.kwargs == dict(slots=2, poll_steps=5)
    got, errors = {}, []

    def client(mine):
        try:
            streams = [(r["name"], b.submit(**r)) for r in mine]
            for name, it in streams:
                got[name] = list(it)
        except Exception as e:                            # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=client, args=(reqs[:4],)), threading.Thread(target=client, args=(reqs[4:],))]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=30)
    assert not errors and sorted(got) == sorted(r["name"] for r in reqs)
    for name, pieces in got.items():
        want = [p for p, _, _ in ref[name] if p is not None]
        assert len(pieces) == len(want)
        for (sr, p), p0 in zip(pieces, want):
            assert sr == 22050 and np.array_equal(p, p0)
    bad = b.submit(name="bad", n=3, ended_by="stop", seed=1, codes=[1, 2, 3], voice="x")
    with pytest.raises(ValueError, match="unknown keys"):
        next(bad)
    b.close()
    assert tts.backend.closed
    with pytest.raises(RuntimeError, match="closed"):
        b.submit(**reqs[0])


def test_stream_batcher_close_and_cancel_end_the_iterators(seven_alone):
    from indextts_amd.serving import StreamBatcher
    reqs, ref = seven_alone
    tts = _FakeSessionTTS()
    b = StreamBatcher(tts, slots=1)
    its = [b.submit(**r) for r in reqs[:3]]
    its[1].cancel()
    b.close()                                             # serves what was submitted, then ends every iterator
    out = [list(it) for it in its]
    assert [len(o) for o in out] == [len(ref["a"]), 0, len(ref["c"])] or len(out[1]) < len(ref["b"])
    assert len(out[0]) == len(ref["a"]) and len(out[2]) == len(ref["c"])
    assert all(next(it, None) is None for it in its) and tts.backend.closed
    tts2 = _FakeSessionTTS()
    b2 = StreamBatcher(tts2, slots=1)
    its2 = [b2.submit(**r) for r in reqs[:3]]
    b2.close(drain=False)
    assert all(len(list(it)) <= len(ref[r["name"]]) for it, r in zip(its2, reqs))   # every iterator ends
    assert tts2.backend.closed
