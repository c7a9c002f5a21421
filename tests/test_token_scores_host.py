"""CPU tests of per-token log-probabilities and best-of-N requests: the C entry's declaration (`itts_gpt_set_token_scores`), the `TokenScores`
record on hand-made arrays, `IndexTTS2.infer_requests(best_of=)` over stand-in stages -- a stub GPT that returns scripted codes and scores --
and the refusals.  The kernel itself is held to the oracle in tests/test_gpu_token_scores.py."""
import math
import os

import pytest
import torch

from indextts_amd import _lib, gpt
from tests.pipeline_stubs import StubFrontend
from tests.test_pipeline_cpu import FakeVoc

STOP = 8193


def test_entry_is_declared_exported_and_bound():
    hdr = open(os.path.join(_lib.HERE, "..", "include", "indextts_hip.h")).read()
    assert "int itts_gpt_set_token_scores(itts_gpt* h, float* logp_model, float* logp_sampled, int n, int max_new);" in hdr
    assert "v13, additive: token scores" in hdr and "#define ITTS_ABI_VERSION 13" in hdr
    comment = hdr[hdr.index("v13, additive: token scores"):hdr.index("int itts_gpt_set_token_scores(")]
    assert "output_scores" in comment and "compute_transition_scores" in comment and "transformers_generation_utils.py:1132" in comment
    assert "F64" in comment or "f64" in comment                                  # the accumulation type is stated
    assert "itts_gpt_set_token_scores" in _lib.SIGNATURES and hasattr(_lib.lib(), "itts_gpt_set_token_scores")
    assert _lib.lib().itts_abi_version() == 13
    assert _lib.lib().itts_gpt_set_token_scores(None, None, None, 0, 0) == _lib.ERR_ARG       # host-only check: no GPU needed


def test_token_scores_lengths_ended_and_means():
    # row 0: the model's own stop at column 2 (cap 6); row 1: runs into its cap of 3 (forced stop at column 3); row 2: no stop in 6 columns;
    # row 3: cap 0 (its first token is forced)
    codes = torch.tensor([[5, 6, STOP, STOP, STOP, STOP],
                          [7, 8, 9, STOP, STOP, STOP],
                          [1, 2, 3, 4, 5, 6],
                          [STOP, STOP, STOP, STOP, STOP, STOP]])
    lengths, ended = gpt.TokenScores.lengths_of(codes, [6, 3, 6, 0], STOP)
    assert lengths.tolist() == [3, 3, 6, 0] and ended.tolist() == [True, False, False, False]
    # a stop token the model chose in its LAST allowed column is its own; one column later it is the cap's
    assert [v.tolist() for v in gpt.TokenScores.lengths_of(torch.tensor([[5, 6, STOP, STOP]]), [3], STOP)] == [[3], [True]]
    assert [v.tolist() for v in gpt.TokenScores.lengths_of(torch.tensor([[5, 6, STOP, STOP]]), [2], STOP)] == [[2], [False]]
    lm = torch.tensor([[-1.0, -2.0, -6.0, 0.0, 0.0, 0.0],
                       [-0.5, -0.25, -0.75, 0.0, 0.0, 0.0],
                       [-1.0, -1.0, -1.0, -1.0, -1.0, -7.0],
                       [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    ls = lm / 2
    ts = gpt.TokenScores(lm, ls, lengths, ended)
    mean, low = ts.mean_logprob(), ts.min_logprob()
    assert mean.dtype == torch.float64 and low.dtype == torch.float64
    assert mean[:3].tolist() == [-3.0, -0.5, -2.0] and low[:3].tolist() == [-6.0, -0.75, -7.0]      # over `lengths` entries only
    assert math.isnan(float(mean[3])) and math.isnan(float(low[3]))                               # nothing of the model's own
    assert ts.mean_logprob("sampled")[:3].tolist() == [-1.5, -0.25, -1.0]
    # the mean is taken in f64 on the host: three f32 values whose f32 sum would round
    v = torch.tensor([[-1e8, -1.0, -1.0]], dtype=torch.float32)
    got = float(gpt.TokenScores(v, v, [3], [False]).mean_logprob()[0])
    assert got == (-1e8 - 2.0) / 3.0
    with pytest.raises(ValueError):
        gpt.TokenScores(lm, ls[:, :3], lengths, ended)
    one = ts.row(1)
    assert one.lengths.tolist() == [3] and one.ended.tolist() == [False] and torch.equal(one.logp_model, lm[1:2])
    st = gpt.TokenScores.stack([ts.row(0), gpt.TokenScores(lm[1:2, :3], ls[1:2, :3], [3], [False])])
    assert st.logp_model.shape == (2, 6) and st.lengths.tolist() == [3, 3] and st.logp_model[1].tolist() == [-0.5, -0.25, -0.75, 0.0, 0.0, 0.0]


def test_generate_refuses_token_scores_with_beams():
    m = object.__new__(gpt.UnifiedVoice)
    m._loaded = True
    with pytest.raises(ValueError, match="token_scores"):
        m.generate(torch.zeros(1, 4, 8), torch.ones(1, 5), 8, num_beams=3, token_scores=True)


# ---- infer_requests over stand-in stages -------------------------------------------------------------------------------------------------
class ScriptedGPT:
    """`inference_speech` returns, for the row whose table entry has stream s, the scripted (codes before the stop, per-token logp, ran into
    its cap) of `script[s]` -- else a default row -- and leaves `last_scores` as the engine does"""
    n_text_pos = 42

    def __init__(self, script=None):
        self.script, self.calls, self.last_scores = script or {}, [], None

    def conds_latent(self, style, emo_vec):
        return torch.zeros(1, 3, 64), None

    @staticmethod
    def _seed(seed, do_sample, uniforms):
        return 7 if seed is None else int(seed)

    def _rows(self, kw):
        rows = []
        for e, cap in zip(kw["row_sampling"], kw["row_max_new"]):
            ids, logp, capped = self.script.get(e["stream"], ([11, 12, 13], [-1.0, -1.0, -1.0, -1.0], False))
            rows.append((list(ids), list(logp), capped))
        return rows

    def inference_speech(self, cond, text, langs, **kw):
        self.calls.append(("inference_speech", text.clone(), kw))
        rows = self._rows(kw)
        W = max(len(ids) + 1 for ids, _, _ in rows)
        codes = torch.full((len(rows), W), STOP, dtype=torch.long)
        lm = torch.zeros(len(rows), W)
        for b, (ids, logp, capped) in enumerate(rows):
            codes[b, : len(ids)] = torch.tensor(ids)
            lm[b, : len(logp)] = torch.tensor(logp)
        self.last_scores = None
        if kw.get("token_scores"):
            self.last_scores = gpt.TokenScores(lm, lm.clone(), [len(logp) for _, logp, _ in rows], [not capped for _, _, capped in rows])
        return codes, None

    def inference_speech_inflight(self, cond, text, langs, slots=8, **kw):
        codes, _ = self.inference_speech(cond, text, langs, **kw)
        self.calls[-1] = ("inference_speech_inflight", text.clone(), dict(kw, slots=slots))
        return codes, None


class RecordingFrontend(StubFrontend):
    def codes_to_mel(self, codes, code_lens, bundle, duration_factor):
        self.calls.append(("codes_to_mel", codes.clone(), code_lens.clone()))
        return super().codes_to_mel(codes, code_lens, bundle, duration_factor)


def _tts(script=None):
    from indextts_amd.infer_v2_5 import IndexTTS2
    return IndexTTS2(cfg={"gpt": {"stop_mel_token": STOP}}, device="cpu", frontend=RecordingFrontend(64), gpt=ScriptedGPT(script), bigvgan=FakeVoc())


REQS = [dict(spk_audio_prompt="a.wav", text="one. two", lang="en", seed=11, best_of=3),
        dict(spk_audio_prompt="b.wav", text="three", lang="en", seed=12, top_k=8, max_mel_tokens=9),
        dict(spk_audio_prompt="a.wav", text="four", lang="en", seed=13, best_of=2)]
C1, C2 = 1 << 16, 2 << 16
# by stream: request 0 segment 0 -> candidates 0 / C1 / C2, segment 1 -> 1 / 1 + C1 / 1 + C2; requests 1 and 2 use stream 0 as well, so the
# script is keyed by values that only request 0's candidates of segment 1 and request 2's candidate 1 carry
SCRIPT = {
    1: ([21, 22], [-0.5, -0.5, -0.5], False),                     # segment 1, candidate 0: ended, mean -0.5
    1 + C1: ([31, 32, 33, 34], [-0.1] * 4, True),                 # candidate 1: the best mean by far, but it ran into its cap
    1 + C2: ([41, 42, 43], [-0.5, -0.25, -0.75, -0.5], False),    # candidate 2: ended, mean -0.5 as well: the tie goes to candidate 0
    C1: ([51, 52, 53, 54, 55], [-0.2] * 6, False),                # request 0 segment 0 candidate 1 AND request 2 candidate 1: the best ended one
}


def test_best_of_expands_rows_chooses_and_renders_only_the_winners():
    t = _tts(SCRIPT)
    outs = t.infer_requests(REQS, num_beams=1, max_mel_tokens=24)
    assert len(outs) == 3 and all(sr == 22050 and w.shape[0] > 0 for sr, w in outs)
    (name, text, kw), = t.gpt.calls
    assert name == "inference_speech" and kw["token_scores"] is True and kw["num_beams"] == 1
    tab = kw["row_sampling"]
    # rows: request 0 segment 0 x 3, request 0 segment 1 x 3, request 1 x 1, request 2 x 2; candidate c of segment j draws from j + (c << 16)
    assert [e["stream"] for e in tab] == [0, C1, C2, 1, 1 + C1, 1 + C2, 0, 0, C1]
    assert [e["seed"] for e in tab] == [11] * 6 + [12] + [13] * 2 and [e["top_k"] for e in tab] == [30] * 6 + [8] + [30] * 2
    assert kw["row_max_new"] == [24] * 6 + [9] + [24] * 2 and kw["max_generate_length"] == 24 and text.shape[0] == 9
    assert kw["conds_latent"].shape[0] == 9
    for lo, hi in ((0, 3), (3, 6), (7, 9)):                         # the candidates of a row share its text
        assert all(torch.equal(text[i], text[lo]) for i in range(lo, hi))
    gpt.row_sampling_entries(tab, 9, dict(do_sample=1, top_k=30, top_p=0.8, temperature=0.8, repetition_penalty=10.0, typical_mass=0.0, seed=5))
    # the choice: greatest mean among the ended; ended beats capped; ties to the lowest candidate
    sc = t.last_scores
    assert [len(s) for s in sc] == [2, 1, 1]
    assert sc[0][0]["chosen"] == 1 and sc[0][0]["mean_logprob"] == pytest.approx([-1.0, -0.2, -1.0]) and sc[0][0]["ended"] == [True] * 3
    assert sc[0][0]["lengths"] == [4, 6, 4]
    assert sc[0][1]["chosen"] == 0 and sc[0][1]["ended"] == [True, False, True] and sc[0][1]["mean_logprob"] == pytest.approx([-0.5, -0.1, -0.5])
    assert sc[1][0] == dict(chosen=0, mean_logprob=[-1.0], lengths=[4], ended=[True])
    assert sc[2][0]["chosen"] == 1 and sc[2][0]["lengths"] == [4, 6]
    # only the winners are rendered, and last_codes holds them
    mel_calls = [c for c in t.frontend.calls if c[0] == "codes_to_mel"]
    rendered = sorted(tuple(c[1][b, : int(c[2][b])].tolist()) for c in mel_calls for b in range(c[1].shape[0]))
    assert rendered == sorted([(51, 52, 53, 54, 55), (21, 22), (11, 12, 13), (51, 52, 53, 54, 55)])
    assert t.last_codes.shape[0] == 4
    assert [t.last_codes[i][t.last_codes[i] != STOP].tolist() for i in range(4)] == [[51, 52, 53, 54, 55], [21, 22], [11, 12, 13], [51, 52, 53, 54, 55]]
    # the same through the in-flight path once the candidate rows are more than the slots
    t2 = _tts(SCRIPT)
    t2.infer_requests(REQS, num_beams=1, max_mel_tokens=24, inflight_slots=4)
    (name2, _, kw2), = t2.gpt.calls
    assert name2 == "inference_speech_inflight" and kw2["slots"] == 4 and [e["stream"] for e in kw2["row_sampling"]] == [e["stream"] for e in tab]
    assert [s[0]["chosen"] for s in t2.last_scores] == [1, 0, 1]


def test_a_capped_winner_is_what_the_cap_warning_speaks_of():
    script = {0: ([1, 2, 3], [-3.0] * 3, True), C1: ([4, 5], [-9.0] * 3, False)}
    t = _tts(script)
    req = dict(spk_audio_prompt="a.wav", text="one", lang="en", seed=1)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)              # the chosen candidate ended on its own: no warning, whatever the loser did
        t.infer_requests([dict(req, best_of=2, max_mel_tokens=3)], num_beams=1)
    assert t.last_scores[0][0]["chosen"] == 1
    with pytest.warns(RuntimeWarning, match="max_mel_tokens"):
        t.infer_requests([dict(req, max_mel_tokens=3)], num_beams=1)


def test_best_of_one_builds_todays_table_and_batch():
    plain = [{k: v for k, v in r.items() if k != "best_of"} for r in REQS]
    calls = []
    for reqs, extra in ((plain, {}), ([dict(r, best_of=1) for r in plain], {}), (plain, dict(best_of=1))):
        t = _tts()
        t.infer_requests(reqs, num_beams=1, max_mel_tokens=24, **extra)
        (name, text, kw), = t.gpt.calls
        assert t.last_scores is None and "token_scores" not in kw
        calls.append((name, text, kw))
    for name, text, kw in calls[1:]:
        assert name == calls[0][0] and torch.equal(text, calls[0][1]) and sorted(kw) == sorted(calls[0][2])
        assert kw["row_sampling"] == calls[0][2]["row_sampling"] and kw["row_max_new"] == calls[0][2]["row_max_new"]
        assert torch.equal(kw["conds_latent"], calls[0][2]["conds_latent"])
    assert [e["stream"] for e in calls[0][2]["row_sampling"]] == [0, 1, 0, 0]
    # token_scores=True in the defaults keeps the scores at best_of = 1, chosen = 0
    t = _tts()
    t.infer_requests(plain, num_beams=1, max_mel_tokens=24, token_scores=True)
    assert t.gpt.calls[0][2]["token_scores"] is True and t.gpt.calls[0][2]["row_sampling"] == calls[0][2]["row_sampling"]
    assert [[s["chosen"] for s in r] for r in t.last_scores] == [[0, 0], [0], [0]] and t.last_scores[1][0]["mean_logprob"] == [-1.0]
    # best_of as a default of the call applies to every request without its own
    t = _tts()
    t.infer_requests([plain[1], dict(plain[2], best_of=1)], num_beams=1, max_mel_tokens=24, best_of=2)
    assert [e["stream"] for e in t.gpt.calls[0][2]["row_sampling"]] == [0, C1, 0]


def test_best_of_refusals():
    req = dict(spk_audio_prompt="a.wav", text="hello", lang="en")
    t = _tts()
    with pytest.raises(ValueError, match="best_of"):                               # beams keep their own hypotheses
        t.infer_requests([dict(req, best_of=2)], num_beams=3)
    with pytest.raises(ValueError, match="best_of"):
        t.infer_requests([req], best_of=2)                                         # (the default num_beams is 3)
    for bad in (0, -1, 2.0, "3", True):
        with pytest.raises(ValueError, match="best_of"):
            t.infer_requests([dict(req, best_of=bad)], num_beams=1)
        with pytest.raises(ValueError, match="best_of"):
            t.infer_requests([req], num_beams=1, best_of=bad)
    assert not t.gpt.calls                                                         # every refusal came before any work
    sess = t.stream_session(slots=2, chunk_size=8, overlap_size=2, max_mel_tokens=24, cfm_noise="global")
    with pytest.raises(ValueError, match="best_of"):
        sess.submit(dict(req, best_of=2))
    assert sess.submit(dict(req, best_of=1)) == 0                                  # 1 is today's stream
    sess.cancel(0)
    sess.close()
    with pytest.raises(ValueError, match="best_of"):
        t.stream_session(slots=2, max_mel_tokens=24, cfm_noise="global", best_of=2)
