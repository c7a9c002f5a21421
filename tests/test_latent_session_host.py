"""CPU tests of the IndexTTS-2 streaming path: the C ABI of the latent session is exported by the cross-compiled library, and the chunk
bookkeeping of `infer_v2.IndexTTS2.infer_stream` -- which codes are appended to the latent session for which chunk, which latents travel with
which chunk, what finished rows are fed -- against a fake `UnifiedVoice` that records every call (no GPU)."""
import numpy as np
import pytest
import torch

from indextts_amd.infer_v2 import ChunkLatents, IndexTTS2 as V2
from tests.pipeline_stubs import StubFrontend

STOP = 8193


def test_library_exports_the_latent_session_abi_13():
    from indextts_amd import _lib
    L = _lib.lib()
    assert L.itts_abi_version() == 13 == _lib.ABI_VERSION
    for name in ("itts_gpt_latent_workspace_bytes", "itts_gpt_latent_open", "itts_gpt_latent_append", "itts_gpt_latent_appended",
                 "itts_gpt_latent_close"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    hdr = open(_lib.HERE + "/../include/indextts_hip.h").read()
    assert "#define ITTS_ABI_VERSION 13" in hdr
    for name in ("itts_gpt_latent_open", "itts_gpt_latent_append", "itts_gpt_latent_close"):
        assert name in hdr
    # null / closed sessions are refused without touching a device
    assert L.itts_gpt_latent_append(None, None, 1, None, None) == _lib.ERR_ARG
    assert L.itts_gpt_latent_close(None) == _lib.ERR_ARG and L.itts_gpt_latent_appended(None) == -1
    assert L.itts_gpt_latent_workspace_bytes(None, 1, 8, 8, 8) == 0


class FakeSession:
    """append() returns latents that name their own (row, mel position, input code): [b, i] = (b, position, code at that position)"""

    def __init__(self, owner, B):
        self.owner, self.B, self.appended, self.closed = owner, B, 0, False
        self.appends = []

    def append(self, codes):
        assert not self.closed and codes.shape[0] == self.B and codes.shape[1] >= 1
        assert codes.shape[1] <= self.owner.session_args["max_append"]
        self.appends.append(codes.clone())
        n = codes.shape[1]
        out = torch.zeros(self.B, n, 8)
        out[:, :, 0] = torch.arange(self.B)[:, None]
        out[:, :, 1] = torch.arange(self.appended, self.appended + n)[None]
        out[:, :, 2] = codes.float()
        self.appended += n
        return out

    def close(self):
        self.closed = True


class FakeVoice:
    """the calls `infer_stream` makes on `UnifiedVoice`, with `generate_chunks` following the engine's chunking rules
    (`UnifiedVoice._generate_chunks_body`) over a fixed code matrix"""
    n_text_pos = 42
    spk_cond_mode = "conformer"

    def __init__(self, lens):
        self.lens = list(lens)
        self.full = torch.full((len(lens), max(lens) + 1), STOP, dtype=torch.long)
        for b, n in enumerate(lens):
            self.full[b, :n] = 100 * (b + 1) + torch.arange(n)
        self.session, self.session_args, self.stream_kw = None, None, None

    def get_conditioning(self, x, lengths=None):
        return torch.ones(1, 32, 8)

    def conds_latent_v2(self, lat, emo):
        return torch.cat([lat + emo[:, None, :8], torch.zeros(lat.shape[0], 2, 8)], 1)

    def latent_conds(self, lat, emo, use_speed=None):
        assert lat.shape[0] == emo.shape[0] == use_speed.shape[0]
        return self.conds_latent_v2(lat, emo)

    def inference_speech_stream(self, cond, text, chunk_size, overlap_size, **kw):
        self.stream_kw = kw
        assert kw["conds_latent"].shape[1:] == (34, 8) and kw["num_beams"] == 1
        return torch.zeros(text.shape[0], 5, 8), torch.ones(text.shape[0], 6), int(kw["max_generate_length"]), {}

    def latent_session(self, conds, text, text_lens, max_codes, max_append):
        assert conds.shape[0] == text.shape[0] == len(text_lens) and conds.shape[1] == 34
        self.session_args = dict(text=text.clone(), text_lens=[int(v) for v in text_lens], max_codes=max_codes, max_append=max_append)
        self.session = FakeSession(self, text.shape[0])
        return self.session

    def generate_chunks(self, emb, mask, max_new, chunk_size, overlap_size, **kw):
        B, stride = len(self.lens), chunk_size - overlap_size
        total = min(max_new, self.full.shape[1])                        # the step that emits the last stop token ends the loop
        codes = torch.full((B, max_new), STOP, dtype=torch.long)
        codes[:, :total] = self.full[:, :total]
        next_at = chunk_size
        while True:
            limit = min(next_at, max_new)
            steps = min(limit, total)
            lens = [min(n, steps) for n in self.lens]
            done = [n < steps for n in self.lens]
            cur = max(lens)
            finished = all(done) or steps >= max_new or steps < limit
            while cur >= next_at:
                pos = next_at - chunk_size
                yield (codes[:, pos:next_at].clone(), False, [d and n <= next_at for d, n in zip(done, lens)],
                       torch.tensor([max(0, min(n - pos, chunk_size)) for n in lens]))
                next_at += stride
            if finished:
                pos = next_at - chunk_size
                if pos < cur:
                    yield (codes[:, pos:cur].clone(), True, [True] * B, torch.tensor([max(0, n - pos) for n in lens]))
                return


class FakeVoc:
    total_up = 256

    def __call__(self, mel, lens=None):
        B, _, T = mel.shape
        w = torch.zeros(B, 1, T * 256)
        for b in range(B):
            w[b, :, : int(lens[b]) * 256] = 0.25
        return w


def _run(lens, chunk, ovl, max_mel=400):
    fe, g = StubFrontend(64), FakeVoice(lens)
    tts = V2(cfg={"gpt": {"stop_mel_token": STOP}, "version": 2.0}, device="cpu", frontend=fe, gpt=g, bigvgan=FakeVoc())
    texts = ["abcdefgh"[: 3 + b] for b in range(len(lens))]
    items = list(tts.infer_stream("spk.wav", texts, chunk_size=chunk, overlap_size=ovl, max_mel_tokens=max_mel, top_k=1))
    return tts, g, texts, items


@pytest.mark.parametrize("lens,chunk,ovl", [([19, 5, 11], 8, 2), ([230, 100, 57], 100, 20),
                                            ([14, 8, 3], 8, 2),            # the longest row ends exactly on a chunk boundary (8 + 6)
                                            ([8, 2], 8, 2), ([180, 100], 100, 20)])
def test_infer_stream_chunk_bookkeeping(lens, chunk, ovl):
    tts, g, texts, items = _run(lens, chunk, ovl)
    B, stride, top = len(lens), chunk - ovl, max(lens)
    sess, recs = g.session, tts.last_stream_latents
    assert sess.closed                                                    # the session ends with the stream
    # the session was opened on the texts WITHOUT the Frontend protocol's stop id, with the stream's budget
    assert g.session_args["text_lens"] == [len(t) for t in texts]
    assert g.session_args["max_codes"] == 400 and g.session_args["max_append"] == chunk
    assert g.stream_kw["max_generate_length"] == 400 and g.stream_kw["do_sample"] is True
    # one record per chunk, chunk k at codes k * stride ...
    assert len(recs) == len(items) and [r["pos"] for r in recs] == [k * stride for k in range(len(recs))]
    appended = 0
    for k, (r, new) in enumerate(zip(recs, sess.appends + [None] * (len(recs) - len(sess.appends)))):
        pos, width = r["pos"], r["codes"].shape[1]
        head = 0 if k == 0 else min(ovl, width)
        assert r["new_from"] == head and r["latent"].shape[:2] == (B, width)
        # appended for this chunk: the first chunk whole, later ones without their overlap head
        assert appended == pos + (0 if k == 0 else ovl)
        if width > head:
            assert torch.equal(new, r["codes"][:, head:])
            appended += width - head
        # the latents that travel with the chunk are those of ITS positions and ITS codes, the head kept from the chunk before
        for b in range(B):
            assert r["latent"][b, :, 0].tolist() == [float(b)] * width
            assert r["latent"][b, :, 1].tolist() == [float(v) for v in range(pos, pos + width)]
            assert torch.equal(r["latent"][b, :, 2].long(), r["codes"][b])
    assert len(sess.appends) == sum(1 for k, r in enumerate(recs) if r["codes"].shape[1] > (0 if k == 0 else ovl))
    assert appended == sess.appended == top                               # every code of the longest row, none twice
    # rows that have ended are fed their stop-token padding
    allc = torch.cat(sess.appends, dim=1)
    for b, n in enumerate(lens):
        assert allc[b, :n].tolist() == [100 * (b + 1) + i for i in range(n)] and (allc[b, n:] == STOP).all()
    # every row finishes exactly once, with int16 mono audio; a finished row yields nothing more
    done_at = [None] * B
    for i, (sr, audio, done) in enumerate(items):
        assert sr == 22050 and len(audio) == B
        for b in range(B):
            if audio[b] is not None:
                assert done_at[b] is None and audio[b].dtype == np.int16 and audio[b].ndim == 1
            if done[b]:
                assert done_at[b] is None
                done_at[b] = i
    assert all(v is not None for v in done_at)
    for b, n in enumerate(lens):           # a row is known to have ended once its stop token exists: the first chunk boundary >= n + 1 codes
        assert done_at[b] == min(len(items) - 1, 0 if n < chunk else -(-(n + 1 - chunk) // stride))


def test_chunk_latents_refuses_a_gap():
    class S:
        def append(self, c):
            return torch.zeros(c.shape[0], c.shape[1], 4)
    t = ChunkLatents(S(), 8, 2)
    t(torch.zeros(2, 8, dtype=torch.long))
    t.appended = 3                                                         # as if codes had been lost between two chunks
    with pytest.raises(RuntimeError, match="appended"):
        t(torch.zeros(2, 8, dtype=torch.long))


def test_v2_infer_stream_is_implemented_and_validates():
    tts, g, texts, items = _run([5, 3], 8, 2)
    assert len(items) >= 1
    with pytest.raises(ValueError, match="overlap_size"):
        list(tts.infer_stream("spk.wav", texts, chunk_size=4, overlap_size=4))
    with pytest.raises(ValueError, match="one segment"):
        list(tts.infer_stream("spk.wav", ["two. segments"], chunk_size=8, overlap_size=2))
    import inspect
    sig = inspect.signature(V2.infer_stream)
    assert "lang" not in sig.parameters and "duration_factor" not in sig.parameters        # the v2 reference has neither
    assert sig.parameters["chunk_size"].default == 100 and sig.parameters["overlap_size"].default == 20
