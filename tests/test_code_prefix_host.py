"""CPU tests of the code-prefix feature's host side: the additive C entries, every refusal `generate(code_prefix=)` /
`inference_speech(input_tokens=)` / `infer_requests` promise, `TokenScores(starts=)`, `IndexTTS2.code_index_at`, the in-flight schedule with
prefixes on a simulated session, and -- on the CPU oracle -- that the decode-rule restatement of tests/code_prefix_ref.py reproduces the plain
run's tail (the resume rule) while the unchanged oracle on cat(fake ids, prefix) does not (the reference rule).  The engine is held to both in
tests/test_gpu_code_prefix.py."""
import os

import pytest
import torch

from indextts_amd import _lib, gpt
from tests import code_prefix_ref as R
from tests.test_inflight_schedule import STOP, _FakeSession, _ids, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert "v13, additive: code prefix" in hdr and "#define ITTS_ABI_VERSION 13" in hdr
    comment = hdr[hdr.index("v13, additive: code prefix"):hdr.index("int itts_gpt_set_code_prefix(")]
    for word in ("input_tokens", "own step", "HOST int32", "Sticky", "ITTS_ERR_STATE", "beam", "itts_gpt_workspace_bytes is unchanged",
                 "not bit-equal", "exactly the launches"):
        assert word in comment, word
    L = _lib.lib()
    for name in ("itts_gpt_set_code_prefix", "itts_gpt_admit_prefix_workspace_bytes", "itts_gpt_last_prefix"):
        assert name in _lib.SIGNATURES and hasattr(L, name) and name + "(" in hdr
    assert L.itts_abi_version() == 13 == _lib.ABI_VERSION
    assert L.itts_gpt_set_code_prefix(None, None, None, 0, 0, 0, 0) == _lib.ERR_ARG          # host-only checks: no GPU needed
    assert L.itts_gpt_admit_prefix_workspace_bytes(None, 1, 4, 3) == 0
    assert L.itts_gpt_last_prefix(None, None, None) == _lib.ERR_ARG
    # the ingest reuses the existing launchers: neither path list has grown
    names = [L.itts_attention_path_name(i).decode() for i in range(L.itts_attention_path_count())]
    assert len(names) == 14 and not any("prefix" in n for n in names)
    assert L.itts_gemm_path_count() == 25 and not any("prefix" in n for n in _lib.gemm_path_names())


def _bare(cls=gpt.UnifiedVoice):
    m = object.__new__(cls)
    m._loaded, m.layers, m.heads, m.kv_cache, m.device = True, 3, 2, True, "cpu"
    m.number_mel_codes, m.stop_mel_token, m.start_mel_token = 100, 99, 98
    return m


def test_generate_refuses_what_it_would_otherwise_get_silently_wrong():
    m = _bare()
    x, mask = torch.zeros(2, 4, 8), torch.ones(2, 5)
    ok = [[1, 2, 3], [4]]
    with pytest.raises(ValueError, match="stop token"):
        m.generate(x, mask, 8, code_prefix=[[1, 99, 3], [4]])
    with pytest.raises(ValueError, match="stop token"):
        m.generate(x, mask, 8, code_prefix=torch.tensor([[1, 2], [99, 5]]))
    with pytest.raises(ValueError, match="cap"):                                    # k_b >= max_new_tokens
        m.generate(x, mask, 3, code_prefix=ok)
    with pytest.raises(ValueError, match="cap"):                                    # ... >= the row's own cap
        m.generate(x, mask, 8, code_prefix=ok, row_max_new=[3, 8])
    with pytest.raises(ValueError, match="outside"):
        m.generate(x, mask, 8, code_prefix=[[1, 100], [4]])
    with pytest.raises(ValueError, match="one sequence per prompt row"):
        m.generate(x, mask, 8, code_prefix=[[1]])
    with pytest.raises(ValueError, match="code_prefix_lens"):
        m.generate(x, mask, 8, code_prefix=torch.tensor([[1, 2], [3, 4]]), code_prefix_lens=[3, 1])
    with pytest.raises(ValueError, match="code_prefix_lens is given without"):
        m.generate(x, mask, 8, code_prefix_lens=[1, 1])
    with pytest.raises(ValueError, match="full width"):                             # uniforms narrower than the full width
        m.generate(x, mask, 8, code_prefix=ok, uniforms=torch.zeros(5, 2, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match="num_beams = 1"):
        m.generate(x, mask, 8, code_prefix=ok, num_beams=3)
    with pytest.raises(ValueError, match="stop token"):
        next(m.generate_chunks(x, mask, 8, 4, 1, code_prefix=[[99], None]))
    with pytest.raises(ValueError, match="prefix_chunk"):
        m._install_prefix((torch.zeros(2, 1, dtype=torch.long), [0, 0]), 0)


def test_input_tokens_travel_in_the_kwargs_and_keep_their_refusals():
    m = _bare()
    m.spk_cond_mode, m.max_mel_tokens = "campplus", 50
    m.prepare_gpt_inputs = lambda conds, text, langs: (None, torch.zeros(2, 4, 8), torch.ones(2, 5))
    conds, text = torch.zeros(2, 3, 8), torch.zeros(2, 6, dtype=torch.long)
    prep = lambda tokens, hf, nret=1: m._prepare_inference(None, text, None, None, None, None, tokens, nret, 8, False, .9, conds, hf)
    out = prep(torch.tensor([5, 6, 7]), dict(do_sample=False))
    assert len(out) == 5                                                            # the 5-tuple the schedule tests stub positionally
    emb, mask, max_new, hf, _ = out
    assert max_new == 8 + 3 and hf["prefix_pos_offset"] == 1 and hf["input_tokens_len"] == 3
    assert hf["code_prefix"].tolist() == [[5, 6, 7]] * 2                            # (s,) serves every row, as the reference repeats it
    assert prep(torch.tensor([[5, 6], [7, 8]]), {})[3]["code_prefix"].tolist() == [[5, 6], [7, 8]]
    assert "code_prefix" not in prep(None, {})[3] and prep(None, {})[2] == 8
    for k, v in (("min_new_tokens", 3), ("begin_suppress_tokens", [4]), ("exponential_decay_length_penalty", (2, 1.1))):
        with pytest.raises(ValueError, match=k):
            prep(torch.tensor([5, 6, 7]), {k: v})
    with pytest.raises(ValueError, match="input_tokens must be"):
        prep(torch.zeros(3, 2, dtype=torch.long), {})
    with pytest.raises(ValueError, match="give one"):
        prep(torch.tensor([5]), dict(code_prefix=[[1], [2]]))
    with pytest.raises(NotImplementedError, match="num_return_sequences"):
        prep(None, {}, nret=2)
    v1 = _bare(gpt.UnifiedVoiceV1)
    with pytest.raises(NotImplementedError, match="v1 pipeline"):
        v1.inference_speech(None, text, input_tokens=torch.tensor([5, 6]))


def test_token_scores_starts():
    lm = torch.tensor([[0.0, 0.0, -1.0, -3.0, 0.0], [-2.0, -4.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0, 0.0]])
    ts = gpt.TokenScores(lm, lm.clone(), [4, 2, 2], [True, False, False], starts=[2, 0, 2])
    assert ts.mean_logprob().tolist()[:2] == [-2.0, -3.0] and ts.min_logprob().tolist()[:2] == [-3.0, -4.0]
    assert ts.mean_logprob()[2] != ts.mean_logprob()[2]                             # nothing generated: nan, as at length 0
    assert gpt.TokenScores(lm, None, [4, 2, 2], [True, False, False]).mean_logprob().tolist()[0] == -1.0      # without starts: all four columns
    assert ts.row(0).starts.tolist() == [2] and ts.row(0).mean_logprob().tolist() == [-2.0]
    st = gpt.TokenScores.stack([ts.row(0), gpt.TokenScores(lm[1:2, :3], lm[1:2, :3].clone(), [2], [False])])
    assert st.starts.tolist() == [2, 0] and st.mean_logprob().tolist() == [-2.0, -3.0]
    assert gpt.TokenScores.stack([gpt.TokenScores(lm[1:2], None, [2], [False])]).starts is None
    with pytest.raises(ValueError, match="starts"):
        gpt.TokenScores(lm, None, [4, 2, 2], [True, False, False], starts=[1, 2])


# ---- the in-flight schedule with prefixes, on a simulated session ---------------------------------------------------------------------------
class _PrefixSession(_FakeSession):
    """`_FakeSession` whose rows may bring given codes: a row with k of them has taken k own steps (`step0` runs k behind), its code row
    starts with them and its ids continue after them"""
    seen = []

    def __init__(self, model, emb, mask, max_new, row_max_new=None, code_prefix=None, prefix_chunk=128, **kw):
        super().__init__(model, emb, mask, max_new, row_max_new=row_max_new, **kw)
        self._place(range(self.B), code_prefix)

    def _place(self, slots, code_prefix):
        """the given codes into the rows' first columns; -> their counts (the simulated rows write own steps >= step0 only: they stay)"""
        ks = []
        for i, b in enumerate(slots):
            p = [] if code_prefix is None or code_prefix[i] is None else [int(v) for v in code_prefix[i]]
            _PrefixSession.seen.append((self.utts[b], p))
            self._codes[b, : len(p)] = torch.tensor(p, dtype=torch.int64)
            self.step0[b] -= len(p)
            ks.append(len(p))
        return ks

    def admit(self, slots, emb, mask, row_max_new=None, code_prefix=None):
        super().admit(slots, emb, mask, row_max_new=row_max_new)                     # (it samples a first id into column 0)
        for b, k in zip(slots, self._place(slots, code_prefix)):                     # ... which, after k given codes, belongs into column k
            u = self.utts[b]
            self._codes[b, k] = _ids(u, self.lens[u])[k] if k < self.lens[u] else STOP


@pytest.mark.parametrize("slots,chunk", [(2, 8), (3, 5), (4, 16)])
def test_inflight_schedule_with_prefixes(monkeypatch, slots, chunk):
    monkeypatch.setattr(gpt, "DecodeSession", _PrefixSession)
    lengths = [30, 3, 6, 17, 40, 8, 8, 9, 25, 12, 5]
    given = [0, 2, 0, 16, 7, 0, 8 - 1, 1, 24, 0, 4]                                 # codes each utterance brings (every one leaves >= 1 to generate)
    prefix = [None if k == 0 else _ids(u, lengths[u])[:k] for u, k in enumerate(given)]
    m = _model(lengths)
    _FakeSession.log, _PrefixSession.seen = [], []
    codes, _ = m.inference_speech_inflight(None, None, max_generate_length=64, slots=slots, chunk_tokens=chunk, do_sample=False, code_prefix=prefix)
    assert codes.shape[0] == len(lengths)
    for u, n in enumerate(lengths):                                                 # complete, in order, each beginning with its prefix
        assert codes[u, :n].tolist() == _ids(u, n) and bool((codes[u, n:] == STOP).all()), u
        assert codes[u, :given[u]].tolist() == (prefix[u] or [])
    assert sorted(_PrefixSession.seen) == sorted((u, prefix[u] or []) for u in range(len(lengths)))      # every prefix reached its own utterance, once
    assert m.last_inflight["admitted"] == len(lengths) - slots
    # without prefixes the schedule passes no such kwarg: the plain simulated session (which takes none) still serves it
    monkeypatch.setattr(gpt, "DecodeSession", _FakeSession)
    plain, _ = m.inference_speech_inflight(None, None, max_generate_length=64, slots=slots, chunk_tokens=chunk, do_sample=False)
    assert torch.equal(plain, codes)
    with pytest.raises(ValueError, match="one entry per utterance"):
        m.inference_speech_inflight(None, None, max_generate_length=64, slots=slots, code_prefix=prefix[:3])


def test_session_counts_given_codes_as_own_steps():
    class M:
        stop_mel_token = STOP
    s = object.__new__(gpt.DecodeSession)
    s.m, s.dev, s.B, s.max_new = M(), "cpu", 2, 8
    s._codes = torch.tensor([[1, 2, 3, 4, STOP, STOP, STOP, STOP],                   # 3 given codes, one generated at session step 1
                             [5, STOP, STOP, STOP, STOP, STOP, STOP, STOP]], dtype=torch.int64)
    s.step0, s.steps = [-3, 0], 1
    assert s.finished() == [] and s.codes(0).tolist() == [1, 2, 3, 4] and s.codes(1).tolist() == [5]
    s.steps = 2
    assert s.finished() == [0, 1] and s.finished_lengths() == [(0, 4), (1, 1)]


# ---- the pipeline's request key ---------------------------------------------------------------------------------------------------------------
def _tts():
    from tests.test_token_scores_host import _tts as build
    return build()


def test_code_prefix_is_a_request_key_and_reaches_the_engine_call():
    t = _tts()
    t.gpt.layers, t.gpt.heads = 3, 2                                                 # (what the alignment-head check reads)
    req = dict(spk_audio_prompt="a.wav", text="one. two", lang="en", seed=11)
    t.infer_requests([dict(req, code_prefix=[[11, 12], None]), dict(req, text="three", code_prefix=[11])], num_beams=1, max_mel_tokens=24)
    (_, _, kw), = t.gpt.calls
    assert kw["code_prefix"] == [[11, 12], None, [11]]                               # one entry per row; a one-segment request may give it bare
    t.gpt.calls.clear()
    t.infer_requests([dict(req, text="three", code_prefix=[11], best_of=2)], num_beams=1, max_mel_tokens=24)
    assert t.gpt.calls[0][2]["code_prefix"] == [[11], [11]]                          # every candidate shares the prefix
    t.gpt.calls.clear()
    t.infer_requests([dict(req, text="three", code_prefix=torch.tensor([11, 12])), dict(req, text="four")], num_beams=1, max_mel_tokens=24,
                     inflight_slots=1)                                               # more rows than slots: the in-flight entry
    assert t.gpt.calls[0][0] == "inference_speech_inflight" and t.gpt.calls[0][2]["code_prefix"] == [[11, 12], None]
    t.gpt.calls.clear()
    t.infer_requests([req], num_beams=1, max_mel_tokens=24)
    assert "code_prefix" not in t.gpt.calls[0][2]                                    # no request brings one: the call is the one it always was
    t.gpt.calls.clear()
    with pytest.raises(ValueError, match=r"unknown keys \['voice'\]"):
        t.infer_requests([dict(req, voice="x")], num_beams=1)
    with pytest.raises(ValueError, match="per segment"):
        t.infer_requests([dict(req, code_prefix=[[11]])], num_beams=1)               # two segments, one entry
    with pytest.raises(NotImplementedError, match="num_beams = 1"):
        t.infer_requests([dict(req, code_prefix=[[11], None])])
    with pytest.raises(ValueError, match="'rescore'"):
        t.infer_requests([dict(req, code_prefix=[[11], None])], num_beams=1, timestamps=True, alignment_heads=[(0, 0)])
    with pytest.raises(ValueError, match="request key"):
        t.infer_requests([req], num_beams=1, code_prefix=[[11], None])               # call-wide: refused
    with pytest.raises(ValueError, match="request key"):
        next(iter(t.infer_stream("a.wav", ["hello"], "en", code_prefix=[[11]])))
    with pytest.raises(ValueError, match="request key"):
        t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global", code_prefix=[[11]])
    with pytest.raises(ValueError, match="request key"):
        t.infer_batch("a.wav", ["hello"], "en", code_prefix=[[11]])
    assert not t.gpt.calls
    from indextts_amd.infer_v2_5 import IndexTTS2

    class V2(IndexTTS2):
        SPK_COND_MODE = "conformer"
    with pytest.raises(NotImplementedError, match="IndexTTS-2.5"):
        object.__new__(V2).infer_requests([dict(req, code_prefix=[[11], None])], num_beams=1)
    from indextts_amd import dist as D
    from indextts_amd.infer import IndexTTS
    with pytest.raises(ValueError, match="request key"):
        IndexTTS._gen_kwargs(dict(code_prefix=[[11]]))
    world = D.world
    D.world = lambda: 2
    try:
        with pytest.raises(NotImplementedError, match="torch.distributed"):
            t.infer_requests([dict(req, code_prefix=[[11], None])], num_beams=1)
    finally:
        D.world = world


def test_stream_submit_refuses_the_key():
    t = _tts()
    sess = t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global")
    with pytest.raises(ValueError, match="unknown keys"):
        sess.submit(dict(spk_audio_prompt="a.wav", text="hello", lang="en", code_prefix=[11]))


def test_code_index_at_inverts_the_timestamp_rule():
    from indextts_amd.infer_v2_5 import IndexTTS2
    t = _tts()
    up = int(t.bigvgan.total_up)
    for dur in (1.0, 1.25, 0.8):
        per = 2 * 1.72 * dur * up
        n_codes, samples = 30, int(30 * 2 * 1.72 * dur) * up
        spans = [(0, 1)] + [(i, i + 1) for i in range(1, n_codes - 1)] + [(n_codes - 1, n_codes)]      # one code per text position
        seg = IndexTTS2.segment_timestamps(spans, list(range(len(spans) - 2)), n_codes, samples, per)
        for j, e in enumerate(seg[1:-1], start=2):                                   # entry of text position j starts where code j starts
            assert t.code_index_at(e["start"], dur) in (j - 1, j) and t.code_index_at(e["start"] + 0.5 * per / 22050, dur) == j
        for i in (0, 1, 7, 29):
            assert t.code_index_at((i * per) / 22050 + 1e-9, dur) == i
            assert t.code_index_at(((i + 1) * per - 1) / 22050, dur) == i
    with pytest.raises(ValueError):
        t.code_index_at(-1.0)


# ---- the two rules on the CPU oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [0, 1, 2, 3])
def test_resume_restatement_reproduces_the_plain_tail_and_the_reference_rule_does_not(golden_dir, si):
    fx = R.fixture(golden_dir)
    s, plain, stop = R.SETS[si], fx["plain"][si], fx["stop"]
    shortest = min(R.n_codes(r, stop) for r in plain)
    for k in sorted({1, min(5, shortest - 1), shortest - 1}):
        new = R.continue_run(fx, s, plain[:, :k], "resume")
        assert torch.equal(new, plain[:, k:]), f"set {si} k {k}: {new.tolist()} vs {plain[:, k:].tolist()}"
    ref = R.continue_run(fx, s, plain[:, :1], "reference")
    w = min(ref.shape[1], plain.shape[1] - 1)
    assert not torch.equal(ref[:, :w], plain[:, 1:1 + w]), "the reference rule is not the plain run's tail"
    assert R.decision_margin(fx["traces"][si], plain, s, fx["uniforms"], stop) >= R.MIN_MARGIN
