"""Host side of the beam sessions (in-flight batching for num_beams > 1): the shared scheduling loop on a SIMULATED beam session, the routing of
`infer_batch(inflight_beam_slots=)` / `DynamicBatcher(inflight_beam_slots=)`, the exported engine entries, and the factored host finaliser
(`gpt.finalize_beam_group`, BeamSearchScorer.finalize, transformers_beam_search.py:320-408) on a scripted search history.  The engine-level contract
is the GPU test tests/test_gpu_beam_session.py."""
import numpy as np
import pytest
import torch

from indextts_amd import gpt, serving, _lib
from indextts_amd.infer_v2_5 import IndexTTS2
from tests.pipeline_stubs import StubFrontend
from tests.test_pipeline_cpu import FakeGPT, FakeVoc

STOP = 99


def _ids(utt, length):
    return [(5 * utt + 3 * t) % 90 for t in range(length)]


class _FakeBeamSession:
    """A group closes (`done`) `lens[u] + 2` steps after it started -- the scorer needs a few steps more than the best hypothesis is long -- or
    stops at its cap; one session step counter, every slot on its own step; the engine's flag check every 4 steps."""
    log = []

    def __init__(self, model, emb, mask, max_new, num_beams=3, row_max_new=None, **kw):
        assert num_beams == 3 and "num_beams" not in kw
        self.utts = [int(v) for v in emb[:, 0, 0].tolist()]
        self.lens = {u: int(emb[i, 0, 1]) for i, u in enumerate(self.utts)}
        self.B, self.max_new, self.steps = len(self.utts), int(max_new), 0
        self.cap = [self.max_new] * self.B if row_max_new is None else [int(c) for c in row_max_new]
        self.step0 = [0] * self.B
        self.S = emb.shape[1] + 1
        _FakeBeamSession.log.append(("open", list(self.utts)))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        _FakeBeamSession.log.append(("close", self.steps))

    def _own(self, b):
        return self.steps - self.step0[b]

    def done(self, b):
        return self._own(b) >= self.lens[self.utts[b]] + 2 and self.lens[self.utts[b]] + 2 <= self.cap[b]

    def finished(self):
        return [b for b in range(self.B) if self.done(b) or self._own(b) >= self.cap[b]]

    def result(self, b):
        u = self.utts[b]
        return torch.tensor(_ids(u, self.lens[u]) if self.done(b) else _ids(u, 400)[:self.cap[b]], dtype=torch.int64)

    def run(self, n, return_when_finished=0):
        limit = self.steps + n if self.steps else min(self.max_new, n)
        while self.steps < limit:
            self.steps += 1
            if self.steps % 4 == 0 and self.steps < limit:
                fin = len(self.finished())
                if fin == self.B or (return_when_finished > 0 and fin >= return_when_finished):
                    break
        return self.steps

    def admit(self, slots, emb, mask, row_max_new=None):
        assert self.steps >= 1 and emb.shape[1] + 1 <= self.S
        for i, b in enumerate(slots):
            assert b in self.finished(), "admitted into a group that is still searching"
            u = int(emb[i, 0, 0])
            self.utts[b], self.lens[u], self.step0[b] = u, int(emb[i, 0, 1]), self.steps - 1
            self.cap[b] = self.max_new if row_max_new is None else int(row_max_new[i])
        _FakeBeamSession.log.append(("admit", list(slots), self.steps))


def _model(lengths, table=400):
    m = object.__new__(gpt.UnifiedVoice)
    m.kv_cache, m.stop_mel_token, m.device = True, STOP, "cpu"
    m._emb = {"mel_pos_embedding.emb.weight": torch.zeros(table + 1, 4)}

    def prep(speech_condition, text_inputs, langs, cond_lengths, emo_vec, campplus_embedding, input_tokens, nret, max_generate_length, *rest):
        n = len(lengths)
        emb = torch.zeros(n, 5, 4)
        emb[:, 0, 0] = torch.arange(n, dtype=torch.float32)
        emb[:, 0, 1] = torch.tensor(lengths, dtype=torch.float32)
        return emb, torch.ones(n, 6, dtype=torch.long), int(max_generate_length), dict(rest[-1]), None
    m._prepare_inference = prep
    return m


@pytest.mark.parametrize("slots,chunk", [(1, 4), (2, 8), (3, 5), (4, 16), (8, 3)])
def test_every_utterance_comes_back_complete_in_order_and_once(monkeypatch, slots, chunk):
    monkeypatch.setattr(gpt, "BeamDecodeSession", _FakeBeamSession)
    lengths = [30, 3, 0, 17, 40, 8, 8, 1, 25, 12, 5]
    m = _model(lengths)
    _FakeBeamSession.log = []
    codes, _ = m.inference_speech_inflight_beams(None, None, max_generate_length=64, slots=slots, chunk_tokens=chunk, do_sample=False)
    assert codes.shape == (len(lengths), max(lengths) + 1)
    for u, n in enumerate(lengths):
        assert codes[u, :n].tolist() == _ids(u, n) and bool((codes[u, n:] == STOP).all()), u
    st = m.last_inflight
    opened = [e for e in _FakeBeamSession.log if e[0] == "open"]
    assert st["sessions"] == len(opened) == 1 and st["truncated"] == 0
    assert st["admitted"] + len(opened[0][1]) == len(lengths)                      # every utterance entered exactly once
    if slots < len(lengths):
        assert st["admitted"] > 0 and len(opened[0][1]) == slots
    assert 0 < st["row_steps"] <= st["slot_steps"] == st["steps"] * min(slots, len(lengths))


def test_caps_free_the_slots_and_count_as_truncated(monkeypatch):
    monkeypatch.setattr(gpt, "BeamDecodeSession", _FakeBeamSession)
    lengths = [50, 6, 6, 50, 6]
    caps = [10, 30, 30, 12, 30]
    m = _model(lengths, table=40)
    codes, _ = m.inference_speech_inflight_beams(None, None, max_generate_length=30, slots=2, chunk_tokens=4, row_max_new=caps, do_sample=False)
    st = m.last_inflight
    assert st["truncated"] == 2 and st["admitted"] == 3 and st["sessions"] == 1
    assert codes[0, :10].tolist() == _ids(0, 400)[:10] and int(codes[0, 10]) == STOP
    assert codes[3, :12].tolist() == _ids(3, 400)[:12] and int(codes[3, 12]) == STOP
    for u in (1, 2, 4):
        assert codes[u, :6].tolist() == _ids(u, 6) and int(codes[u, 6]) == STOP
    with pytest.raises(ValueError):
        m.inference_speech_inflight_beams(None, None, max_generate_length=41, slots=2)
    with pytest.raises(ValueError):
        m.inference_speech_inflight_beams(None, None, max_generate_length=30, slots=2, num_beams=1)
    with pytest.raises(ValueError):                              # a beam search runs at least its first step
        m.inference_speech_inflight_beams(None, None, max_generate_length=30, slots=2, row_max_new=[10, 0, 30, 12, 30])
    with pytest.raises(NotImplementedError):                     # the num_beams = 1 call keeps refusing beams
        m.inference_speech_inflight(None, None, max_generate_length=30, slots=2, num_beams=3)


def test_infer_batch_routes_beam_groups_through_the_beam_inflight_call():
    class GPT(FakeGPT):
        def __init__(self):
            super().__init__()
            self.beams, self.inflight = [], []

        def inference_speech_inflight_beams(self, cond, text, langs, slots=None, chunk_tokens=16, min_free=1, num_beams=3, **kw):
            self.beams.append((text.shape[0], slots, chunk_tokens, min_free, num_beams, kw))
            return FakeGPT.inference_speech(self, cond, text, langs, **kw)

        def inference_speech_inflight(self, cond, text, langs, slots=None, chunk_tokens=16, min_free=1, **kw):
            self.inflight.append(text.shape[0])
            return FakeGPT.inference_speech(self, cond, text, langs, **kw)

    tts = IndexTTS2(cfg={"gpt": {"stop_mel_token": 8193}}, device="cpu", frontend=StubFrontend(64), gpt=GPT(), bigvgan=FakeVoc())
    texts = ["one.", "two two.", "three three three.", "four.", "five five."]
    out = tts.infer_batch("spk.wav", texts, "en", inflight_beam_slots=2, chunk_tokens=8, min_free=2)          # the default 3 beams
    assert len(out) == 5 and len(tts.gpt.beams) == 1
    n, slots, chunk, min_free, nb, kw = tts.gpt.beams[0]
    assert (n, slots, chunk, min_free, nb) == (5, 2, 8, 2, 3)
    assert not {"inflight_beam_slots", "inflight_slots", "chunk_tokens", "min_free"} & set(kw)
    plain = len(tts.gpt.calls)
    tts.infer_batch("spk.wav", texts, "en", num_beams=3, inflight_slots=2)           # `inflight_slots` with beams stays the plain batch call
    tts.infer_batch("spk.wav", texts, "en", num_beams=3, inflight_beam_slots=8)      # everything fits the groups: one ordinary batch
    tts.infer_batch("spk.wav", texts, "en", num_beams=1, inflight_beam_slots=2)      # no beams: not this path
    assert len(tts.gpt.beams) == 1 and not tts.gpt.inflight and len(tts.gpt.calls) == plain + 3
    for _, kw in tts.gpt.calls[plain:]:
        assert "inflight_beam_slots" not in kw and "inflight_slots" not in kw


def test_dynamic_batcher_forwards_inflight_beam_slots():
    class TTS:
        def __init__(self):
            self.seen = []

        def infer_batch(self, spk, texts, lang, **kw):
            self.seen.append(dict(kw))
            return [(22050, np.zeros(4, dtype=np.int16)) for _ in texts]

    tts = TTS()
    b = serving.DynamicBatcher(tts, max_batch=4, max_wait_ms=1.0, inflight_slots=8, inflight_beam_slots=3)
    try:
        b.submit("spk.wav", "default beams", "en").result(timeout=30)
        b.submit("spk.wav", "one beam", "en", num_beams=1).result(timeout=30)
        b.submit("spk.wav", "own setting", "en", num_beams=2, inflight_beam_slots=5).result(timeout=30)
    finally:
        b.close()
    by = {kw.get("num_beams", 3): kw for kw in tts.seen}
    assert by[3].get("inflight_beam_slots") == 3 and "inflight_slots" not in by[3]
    assert by[1].get("inflight_slots") == 8 and "inflight_beam_slots" not in by[1]
    assert by[2]["inflight_beam_slots"] == 5


def test_beam_session_entries_are_declared_and_exported():
    import os
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "indextts_hip.h")).read()
    for name in ("itts_gpt_generate_beam_chunk", "itts_gpt_admit_beam_workspace_bytes", "itts_gpt_admit_beam_groups"):
        assert hasattr(L, name) and name in _lib.SIGNATURES and name + "(" in hdr
    assert "v13, additive: beam sessions" in hdr and L.itts_abi_version() == 13 == _lib.ABI_VERSION


def _old_generate_beam_finalize(ht, hp, bs, hy_s, hy_i, nh, dn, steps_run, nb, length_penalty):
    """`UnifiedVoice._generate_beam`'s host finalisation as it stood before it was factored out (whole batch at once)."""
    B = len(dn)
    if dn.all():
        last = max(int(hy_i[b, q, 1]) for b in range(B) for q in range(int(nh[b])))
        steps_run = min(steps_run, last + 1)

    def seq_of(row, upto):
        toks, r = [], row
        for sidx in range(upto, -1, -1):
            toks.append(int(ht[sidx, r]))
            r = int(hp[sidx, r])
        return toks[::-1]
    best = []
    for b in range(B):
        heap = [(float(hy_s[b, q, 0]), seq_of(int(hy_i[b, q, 2]), int(hy_i[b, q, 1]) - 1) if int(hy_i[b, q, 1]) > 0 else []) for q in range(int(nh[b]))]
        if not dn[b]:
            worst = min([h0[0] for h0 in heap], default=1e9) if len(heap) >= nb else 1e9
            for j in range(nb):
                row = b * nb + j
                sc = float(bs[row]) / (steps_run ** float(length_penalty))
                if len(heap) < nb or sc > worst:
                    heap.append((sc, seq_of(row, steps_run - 1)))
                    if len(heap) > nb:
                        heap.remove(min(heap, key=lambda t: t[0]))
                    worst = min(t[0] for t in heap)
        best.append(sorted(heap, key=lambda t: t[0])[-1][1])
    return best


@pytest.mark.parametrize("length_penalty", [0.0, 1.0])
def test_factored_finaliser_gives_generate_beams_old_output(length_penalty):
    """A scripted 3-utterance, 3-beam history of 6 steps: utterance 0 is done with its best hypothesis ended at step 2 (before the last step),
    utterance 1 is NOT done (one finished hypothesis, the open beams compete with it), utterance 2 is done with a hypothesis that ended at step 0
    (empty sequence) losing to a later one."""
    nb, B, steps = 3, 3, 6
    rng = np.random.RandomState(5)
    ht = rng.randint(0, 90, size=(steps, B * nb)).astype(np.int32)
    hp = np.stack([np.repeat(np.arange(B), nb) * nb + rng.randint(0, nb, size=B * nb) for _ in range(steps)]).astype(np.int32)
    bs = np.array([0, 0, 0, -2.0, -3.5, -9.0, 0, 0, 0], dtype=np.float32)
    hy_s = np.zeros((B, 4, 4), dtype=np.float32)
    hy_i = hy_s.view(np.int32)
    nh = np.array([3, 1, 3], dtype=np.int32)
    dn = np.array([1, 0, 1], dtype=np.uint8)
    for b, recs in {0: [(-1.0, 2, 1), (-4.0, 4, 0), (-2.5, 5, 2)], 1: [(-3.0, 3, 5)], 2: [(-6.0, 0, 6), (-1.5, 4, 8), (-2.0, 3, 7)]}.items():
        for q, (score, step, row) in enumerate(recs):
            hy_s[b, q, 0] = score
            hy_i[b, q, 1], hy_i[b, q, 2] = step, row
    want = _old_generate_beam_finalize(ht, hp, bs, hy_s, hy_i, nh, dn, steps, nb, length_penalty)
    steps_run = gpt.beam_steps_run(hy_s, nh, dn, steps)
    assert steps_run == steps                                   # an utterance is not done: the loop ran to max_length
    got = [gpt.finalize_beam_group(ht, hp, bs, hy_s, nh, dn, steps_run, length_penalty, group=b, num_beams=nb) for b in range(B)]
    assert got == want
    assert len(got[0]) == 2 and len(got[1]) in (3, steps) and len(got[2]) == 4
    # every utterance done: the reference loop ended right after the last hypothesis closed
    dn2 = np.array([1, 1, 1], dtype=np.uint8)
    assert gpt.beam_steps_run(hy_s, nh, dn2, steps) == 6 and gpt.beam_steps_run(hy_s, nh, dn2, 4) == 4
    hy_i[0, 2, 1] = 3
    assert gpt.beam_steps_run(hy_s, nh, dn2, steps) == 5
