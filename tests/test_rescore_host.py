"""CPU tests of the rescoring pass's host side: the additive C entries' declarations (`itts_gpt_rescore`, its workspace query and the two unit
entries), `TokenScores` without `logp_sampled`, and `IndexTTS2.infer_requests(timestamps="rescore" / token_scores="rescore")` over stand-in
stages -- a stub GPT that returns scripted codes under ANY num_beams and records the one batched `inference_speech_rescore` call -- with
every refusal the earlier tests pin.  The kernels are held to their references in tests/test_gpu_rescore_kernels.py, the pass in
tests/test_gpu_rescore.py."""
import os

import pytest
import torch

from indextts_amd import _lib, gpt
from tests.test_alignment_host import HEADS, SPC, STOP, UP, AlignedGPT, _expected_segment
from tests.test_pipeline_cpu import FakeVoc
from tests.test_token_scores_host import RecordingFrontend


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(_lib.HERE, "..", "include", "indextts_hip.h")).read()
    assert "v13, additive: rescoring pass" in hdr and "#define ITTS_ABI_VERSION 13" in hdr
    comment = hdr[hdr.index("v13, additive: rescoring pass"):hdr.index("size_t itts_gpt_rescore_workspace_bytes(")]
    for word in ("UnifiedVoice.forward", "get_logits", "compute_transition_scores", "output_attentions=True", "Row 0 IS written", "suspended",
                 "No graph capture", "HOST int32", "grows with chunk"):
        assert word in comment, word
    L = _lib.lib()
    for name in ("itts_gpt_rescore_workspace_bytes", "itts_gpt_rescore", "itts_gpt_logp_gather_forward", "itts_gpt_attention_align_mq_forward"):
        assert name in _lib.SIGNATURES and hasattr(L, name) and name + "(" in hdr
    assert L.itts_abi_version() == 13 == _lib.ABI_VERSION
    # host-only checks: no GPU needed
    assert L.itts_gpt_rescore_workspace_bytes(None, 1, 4, 8, 4) == 0
    assert L.itts_gpt_rescore(None, None, None, 1, 4, None, None, 8, 2, None, None, 0, None, None, 0, 4, None, 0, None) == _lib.ERR_ARG
    assert L.itts_gpt_logp_gather_forward(None, None, None, 3, 5, 8, None) == _lib.ERR_ARG
    assert L.itts_gpt_attention_align_mq_forward(*([None] * 5), 1, *([None] * 5), 1, 2, 3, 8, 1, 0, 3, 8, 0, None) == _lib.ERR_ARG
    # neither kernel is a path of launch_attention / launch_gemm: the lists and their counts are what they were
    names = [L.itts_attention_path_name(i).decode() for i in range(L.itts_attention_path_count())]
    assert len(names) == 14 and not any("align" in n or "mq" in n for n in names)
    assert L.itts_gemm_path_count() == 25 and not any("logp" in n for n in _lib.gemm_path_names())


def test_token_scores_without_logp_sampled():
    lm = torch.tensor([[-1.0, -3.0, 0.0], [-2.0, 0.0, 0.0]])
    ts = gpt.TokenScores(lm, None, [2, 1], [True, False])
    assert ts.mean_logprob().tolist() == [-2.0, -2.0] and ts.min_logprob().tolist() == [-3.0, -2.0]
    with pytest.raises(ValueError, match="logp_sampled"):
        ts.mean_logprob("sampled")
    assert ts.row(1).logp_sampled is None and ts.row(1).lengths.tolist() == [1]
    st = gpt.TokenScores.stack([ts.row(0), gpt.TokenScores(lm[1:2, :2], None, [1], [False])])
    assert st.logp_sampled is None and st.logp_model.shape == (2, 3)
    with pytest.raises(ValueError):
        gpt.TokenScores(lm, None, [2], [True])


# ---- infer_requests over stand-in stages -------------------------------------------------------------------------------------------------
class RescoreGPT(AlignedGPT):
    """AlignedGPT that also decodes beam calls (no per-row table there: the row index is the stream) and records `inference_speech_rescore`,
    which leaves a staircase over the codes it is GIVEN -- row 0 included, as the rescoring pass writes it"""
    stop_mel_token = STOP

    def inference_speech(self, cond, text, langs, **kw):
        if "row_sampling" not in kw:
            kw = dict(kw, row_sampling=[dict(stream=b) for b in range(text.shape[0])])
        return super().inference_speech(cond, text, langs, **kw)

    def inference_speech_inflight_beams(self, cond, text, langs, slots=8, **kw):
        kw.pop("chunk_tokens", None), kw.pop("min_free", None)
        out = self.inference_speech(cond, text, langs, **kw)
        self.calls[-1] = ("inference_speech_inflight_beams",) + self.calls[-1][1:]
        return out

    def inference_speech_rescore(self, cond, text, codes, **kw):
        self.calls.append(("inference_speech_rescore", text.clone(), dict(kw, codes=codes.clone())))
        T = [int(((t != 0) & (t != 1)).sum()) + 2 for t in text]
        lens = [int(v) for v in kw["code_lens"]]
        B, W = codes.shape
        lm = torch.zeros(B, W)
        for b in range(B):
            lm[b, : lens[b]] = -0.25 * (b + 1)
        ts = gpt.TokenScores(lm, None, lens, [True] * B)
        al = None
        if kw.get("alignment_heads") is not None:
            attn = torch.zeros(B, W, len(kw["alignment_heads"]), max(T))
            for b in range(B):
                n = lens[b] - 1                             # codes before the stop token
                attn[b, 0, :, 0] = 1.0
                for i in range(1, n + 1):
                    attn[b, i, :, min(T[b] - 1, i * T[b] // n)] = 1.0
            al = gpt.TokenAlignment(attn, T, lens)
        return ts, al


def _tts():
    from indextts_amd.infer_v2_5 import IndexTTS2
    return IndexTTS2(cfg={"gpt": {"stop_mel_token": STOP}}, device="cpu", frontend=RecordingFrontend(64), gpt=RescoreGPT(), bigvgan=FakeVoc())


REQS = [dict(spk_audio_prompt="a.wav", text="abcd. efghijk", lang="en", duration_factor=1.25),
        dict(spk_audio_prompt="b.wav", text="xyz", lang="en")]


@pytest.mark.parametrize("beams", [dict(num_beams=3), dict(), dict(num_beams=3, beam_settings="own"), dict(num_beams=3, inflight_beam_slots=2),
                                   dict(num_beams=1), dict(num_beams=1, inflight_slots=2)])
def test_rescore_timestamps_reach_the_engine_once_for_the_whole_batch(beams):
    t = _tts()
    plain = t.infer_requests(REQS, max_mel_tokens=40, interval_silence=100, **beams)
    codes_plain = t.last_codes.clone()
    assert t.last_timestamps is None and t.last_scores is None and [c[0] for c in t.gpt.calls].count("inference_speech_rescore") == 0
    t.gpt.calls.clear()
    outs = t.infer_requests(REQS, max_mel_tokens=40, timestamps="rescore", alignment_heads=HEADS, interval_silence=100, **beams)
    names = [c[0] for c in t.gpt.calls]
    assert names.count("inference_speech_rescore") == 1 and len(names) == 2, names           # ONE pass for the three segments of both requests
    decode_kw = t.gpt.calls[0][2]
    assert "timestamps" not in decode_kw and "alignment_heads" not in decode_kw and "token_scores" not in decode_kw
    assert decode_kw["num_beams"] == beams.get("num_beams", 3)
    _, text, kw = t.gpt.calls[1]
    assert text.shape[0] == 3 and kw["alignment_heads"] == HEADS and torch.equal(kw["codes"], t.last_codes)
    assert kw["code_lens"] == [int((row != STOP).sum()) + 1 for row in t.last_codes]            # up to and including the first stop token
    # the codes and the audio are those of the call without the kwarg
    assert torch.equal(t.last_codes, codes_plain)
    assert all(a[0] == b[0] and (a[1] == b[1]).all() for a, b in zip(outs, plain))
    # the timestamps: the staircase of the stub by the existing timing rule (row 0 carries attention here; it is pinned to position 0 anyway)
    ts = t.last_timestamps
    assert [len(r) for r in ts] == [2, 1]
    sil, offset = int(22050 * 100 / 1000.0), 0
    for seg, n_ids in zip(ts[0], (4, 7)):
        n_codes = 2 * (n_ids + 2)
        rendered = int(n_codes * 2 * 1.25) * UP
        want = _expected_segment(n_ids, n_codes, 1.25, offset, rendered)
        for e, (a, b) in zip(seg, want):
            assert e["start"] == pytest.approx(a, abs=1e-12) and e["end"] == pytest.approx(b, abs=1e-12), (seg, want)
        offset += rendered + sil
    assert ts[1][0][0]["start"] == 0.0 and ts[1][0][-1]["end"] == pytest.approx(outs[1][1].shape[0] / 22050)
    # ... and the scores of the same pass
    sc = t.last_scores
    assert [len(r) for r in sc] == [2, 1]
    assert [s["mean_logprob"] for r in sc for s in r] == [-0.25, -0.5, -0.75] and [s["lengths"] for r in sc for s in r] == kw["code_lens"]


def test_rescore_scores_alone_ask_for_no_heads_and_the_attribute_serves_the_kwarg():
    t = _tts()
    t.infer_requests(REQS, num_beams=3, max_mel_tokens=40, token_scores="rescore")
    (_, _, kw), = [c for c in t.gpt.calls if c[0] == "inference_speech_rescore"]
    assert kw["alignment_heads"] is None and t.last_timestamps is None
    assert [s["mean_logprob"] for r in t.last_scores for s in r] == [-0.25, -0.5, -0.75]
    t.alignment_heads = HEADS
    t.infer_requests(REQS, num_beams=3, max_mel_tokens=40, timestamps="rescore")
    assert t.gpt.calls[-1][0] == "inference_speech_rescore" and t.gpt.calls[-1][2]["alignment_heads"] == HEADS and t.last_timestamps is not None
    # beside a best_of report the rescored numbers get keys of their own
    t.infer_requests([dict(REQS[1], best_of=2)], num_beams=1, max_mel_tokens=40, token_scores="rescore")
    d = t.last_scores[0][0]
    assert d["chosen"] in (0, 1) and len(d["mean_logprob"]) == 2 and d["rescored_mean_logprob"] == -0.25 and d["rescored_lengths"] > 0


def test_refusals_stay_and_come_before_any_engine_work():
    req = dict(spk_audio_prompt="a.wav", text="hello", lang="en")
    t = _tts()
    for key in ("timestamps", "token_scores"):
        for bad in ("rescored", "Rescore", "true", ""):
            with pytest.raises(ValueError, match="'rescore'") as e:
                t.infer_requests([req], num_beams=3, alignment_heads=HEADS, **{key: bad})
            assert "True" in str(e.value)                                           # the two accepted values are named
    with pytest.raises(ValueError, match="alignment_heads"):                         # no default list is shipped
        t.infer_requests([req], timestamps="rescore")
    with pytest.raises(ValueError, match="alignment_heads"):
        t.infer_requests([req], timestamps="rescore", alignment_heads=[(3, 0)])
    # `timestamps=True` keeps its meaning and its refusals, word for word
    with pytest.raises(ValueError, match=r"timestamps=True applies to num_beams = 1 only \(got num_beams = 3\)"):
        t.infer_requests([req], num_beams=3, timestamps=True, alignment_heads=HEADS)
    with pytest.raises(ValueError, match="num_beams"):
        t.infer_requests([req], timestamps=True, alignment_heads=HEADS)
    with pytest.raises(ValueError, match="token_scores=True is implemented for num_beams = 1 only"):
        t.infer_requests([req], num_beams=3, token_scores=True)
    with pytest.raises(ValueError, match="alignment_heads is given without timestamps=True"):
        t.infer_requests([req], num_beams=3, alignment_heads=HEADS)
    with pytest.raises(ValueError, match="alignment_heads is given without timestamps=True"):
        t.infer_requests([req], num_beams=3, token_scores="rescore", alignment_heads=HEADS)
    # streams
    with pytest.raises(ValueError, match="timestamps"):
        next(iter(t.infer_stream("a.wav", ["hello"], "en", timestamps="rescore")))
    with pytest.raises(ValueError, match="timestamps"):
        t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global", timestamps="rescore")
    # the v2 / v1 pipelines and torch.distributed
    from indextts_amd.infer_v2_5 import IndexTTS2

    class V2(IndexTTS2):
        SPK_COND_MODE = "conformer"
    v2 = object.__new__(V2)
    with pytest.raises(NotImplementedError, match="IndexTTS-2.5"):
        v2.infer_requests([req], timestamps="rescore", alignment_heads=HEADS)
    from indextts_amd import dist as D
    world = D.world
    D.world = lambda: 2
    try:
        with pytest.raises(NotImplementedError, match="torch.distributed"):
            t.infer_requests([req], timestamps="rescore", alignment_heads=HEADS)
    finally:
        D.world = world
    assert not t.gpt.calls and not t.frontend.calls                                 # every refusal came before any work
    # the engine's Python entries (which the v2 and v1 pipelines forward their kwargs to) do not take the pipeline's kwarg in any spelling
    m = object.__new__(gpt.UnifiedVoice)
    m._loaded, m.layers, m.heads = True, 3, 2
    x, mask = torch.zeros(2, 4, 8), torch.ones(2, 5)
    with pytest.raises(ValueError, match="infer_requests"):
        m.generate(x, mask, 8, timestamps="rescore")
    with pytest.raises(ValueError, match="infer_requests"):
        next(m.generate_chunks(x, mask, 8, 4, 1, timestamps="rescore"))
    # `rescore` checks its arguments before it touches a handle (the object has none)
    codes = torch.zeros(2, 6, dtype=torch.long)
    with pytest.raises(ValueError, match="codes"):
        m.rescore(x, mask, codes[:1])
    with pytest.raises(ValueError, match="chunk"):
        m.rescore(x, mask, codes, chunk=0)
    with pytest.raises(ValueError, match="chunk"):
        m.rescore(x, mask, codes, chunk=65536)
    with pytest.raises(ValueError, match="alignment_heads"):
        m.rescore(x, mask, codes, alignment_heads=[(3, 0)], text_spans=[(0, 2), (0, 2)])
    with pytest.raises(ValueError, match="text_spans"):
        m.rescore(x, mask, codes, alignment_heads=HEADS)
    with pytest.raises(ValueError, match="text_spans"):
        m.rescore(x, mask, codes, text_spans=[(0, 2), (0, 2)])
    m.device, m.stop_mel_token = "cpu", STOP
    with pytest.raises(ValueError, match="code_lens"):
        m.rescore(x, mask, codes, code_lens=[7, 1])
    with pytest.raises(ValueError, match="code_lens"):
        m.rescore(x, mask, codes, code_lens=[1])
