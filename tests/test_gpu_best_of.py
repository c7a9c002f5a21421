"""Best-of-N requests on the real HIP engines (tiny random models, the pipeline shape of tests/test_gpu_mixed_requests.py with a stand-in
codes -> mel): `IndexTTS2.infer_requests(best_of=N)` decodes every segment as N candidate rows of the one GPT batch, scores them with the
token selection kernel's per-token log-probabilities, and renders only the winner.  Every candidate is the row a direct
`inference_speech(..., row_sampling=[entry with stream = j + (c << 16)], token_scores=True)` decodes alone -- ids and score bits -- so a
request's chosen codes depend on nothing but the request."""
import warnings

import numpy as np
import pytest
import torch

from tests.test_gpu_mixed_requests import VoiceFrontend
from tests.test_gpu_pipeline import build

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOP = 8193
KW = dict(num_beams=1, max_mel_tokens=24)
REQS = [
    dict(spk_audio_prompt="alice.wav", text="hello world. a much longer second sentence here", lang="en", seed=21, temperature=1.0, top_p=0.95),
    dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=22, temperature=1.2, top_p=1.0, top_k=20, max_mel_tokens=9),
    dict(spk_audio_prompt="alice.wav", text="one more for the first voice", lang="en", seed=23, repetition_penalty=2.0),
]


@pytest.fixture(scope="module")
def tts():
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    return t


def _run(tts, reqs, **kw):
    """-> (waveforms, per request the list of its segments' chosen ids up to the stop token, last_scores, the GPT call's (text, langs, kwargs))"""
    seen = []
    real, real_inflight = tts.gpt.inference_speech, tts.gpt.inference_speech_inflight

    def spy(cond, text, langs, **k):
        seen.append((text.clone(), langs.clone(), dict(k)))
        return real(cond, text, langs, **k)

    def spy_inflight(cond, text, langs, **k):
        seen.append((text.clone(), langs.clone(), dict(k)))
        return real_inflight(cond, text, langs, **k)
    tts.gpt.inference_speech, tts.gpt.inference_speech_inflight = spy, spy_inflight
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # (a chosen candidate may have run into its max_mel_tokens)
            outs = tts.infer_requests(reqs, **kw)
    finally:
        del tts.gpt.inference_speech, tts.gpt.inference_speech_inflight
    codes = tts.last_codes.cpu()
    sc = tts.last_scores
    per_req, i = [], 0
    for r in range(len(reqs)):
        n_seg = len(sc[r]) if sc is not None else None
        if n_seg is None:
            n_seg = len([s for s in reqs[r]["text"].split(".") if s.strip()])
        per_req.append([codes[i + j][codes[i + j] != STOP].tolist() for j in range(n_seg)])
        i += n_seg
    assert i == codes.shape[0]
    return outs, per_req, sc, seen[0]


def _rule(means, ended):
    """the selection rule, restated: ended before capped, then the greatest mean, then the lowest index"""
    order = sorted(range(len(means)), key=lambda c: (not ended[c], -(means[c] if means[c] == means[c] else float("-inf")), c))
    return order[0]


def test_every_candidate_is_its_row_alone_and_the_winner_follows_the_rule(tts):
    outs, chosen_codes, sc, (text, langs, kw) = _run(tts, REQS, best_of=3, **KW)
    tab, caps = kw["row_sampling"], kw["row_max_new"]
    assert text.shape[0] == 12 and len(tab) == 12 and kw["token_scores"] is True        # 4 segments x 3 candidates in ONE batch
    assert [e["stream"] for e in tab] == [j + (c << 16) for j in (0, 1) for c in range(3)] + [c << 16 for c in range(3)] * 2
    assert [e["seed"] for e in tab] == [21] * 6 + [22] * 3 + [23] * 3 and caps == [24] * 6 + [9] * 3 + [24] * 3
    rows = [(0, 0), (0, 1), (1, 0), (2, 0)]
    n_distinct = 0
    for i, (r, j) in enumerate(rows):
        rec = sc[r][j]
        cand = []
        for c in range(3):
            m = 3 * i + c
            ids, _ = tts.gpt.inference_speech(None, text[m:m + 1], langs[m:m + 1], conds_latent=kw["conds_latent"][m:m + 1], do_sample=True, num_beams=1,
                                              length_penalty=kw["length_penalty"], max_generate_length=kw["max_generate_length"], row_max_new=[caps[m]],
                                              row_sampling=[dict(tab[m], stream=j + (c << 16))], token_scores=True)
            one = tts.gpt.last_scores
            mean = float(one.mean_logprob()[0])
            assert rec["mean_logprob"][c] == mean, f"request {r} segment {j} candidate {c}: {rec['mean_logprob'][c]!r} in the batch, {mean!r} alone"
            assert rec["lengths"][c] == int(one.lengths[0]) and rec["ended"][c] == bool(one.ended[0])
            cand.append(ids[0].cpu()[ids[0].cpu() != STOP].tolist())
        n_distinct += len({tuple(v) for v in cand})
        want = _rule(rec["mean_logprob"], rec["ended"])
        print(f"request {r} segment {j}: means {[round(v, 4) for v in rec['mean_logprob']]} ended {rec['ended']} lengths {rec['lengths']} -> {rec['chosen']}")
        assert rec["chosen"] == want
        assert chosen_codes[r][j] == cand[want], f"request {r} segment {j}: last_codes is not candidate {want}'s ids"
    assert n_distinct >= 8, "the candidates of a row must differ, or choosing among them shows nothing"
    assert len(outs) == 3 and all(sr == 22050 and w.dtype == np.int16 and w.shape[0] > 0 for sr, w in outs)


def test_the_choice_does_not_depend_on_order_or_batch_mates(tts):
    _, base, sc, _ = _run(tts, REQS, best_of=3, **KW)
    _, rev, sc_rev, _ = _run(tts, REQS[::-1], best_of=3, **KW)
    extra = dict(spk_audio_prompt="carol.wav", text="an unrelated request. of two segments", lang="en", seed=99, best_of=2)
    _, more, sc_more, _ = _run(tts, [extra] + REQS, best_of=3, **KW)
    for r in range(3):
        assert rev[2 - r] == base[r] and more[r + 1] == base[r], f"request {r}: its chosen codes changed with the batch"
        assert sc_rev[2 - r] == sc[r] and sc_more[r + 1] == sc[r], f"request {r}: its scores changed with the batch"
    assert len(sc_more[0]) == 2 and all(len(s["mean_logprob"]) == 2 for s in sc_more[0])


def test_best_of_one_is_the_call_without_the_key(tts):
    outs0, codes0, sc0, (_, _, kw0) = _run(tts, REQS, **KW)
    outs1, codes1, sc1, (_, _, kw1) = _run(tts, [dict(r, best_of=1) for r in REQS], **KW)
    assert sc0 is None and sc1 is None and "token_scores" not in kw1 and kw1["row_sampling"] == kw0["row_sampling"]
    assert codes1 == codes0
    for (sr0, w0), (sr1, w1) in zip(outs0, outs1):
        assert sr0 == sr1 and w0.shape == w1.shape and np.array_equal(w0, w1)
    # ... and candidate 0 of a best-of-3 call is that row
    _, _, sc3, (text, langs, kw3) = _run(tts, REQS, best_of=3, **KW)
    _, scored, sc_plain, _ = _run(tts, REQS, token_scores=True, **KW)
    assert scored == codes0 and [[s["chosen"] for s in r] for r in sc_plain] == [[0, 0], [0], [0]]
    for r in range(3):
        for j in range(len(sc3[r])):
            assert sc_plain[r][j]["mean_logprob"][0] == sc3[r][j]["mean_logprob"][0]


def test_best_of_through_the_inflight_path(tts):
    _, base, sc, (_, _, kw) = _run(tts, REQS, best_of=3, **KW)
    _, got, sc_in, (_, _, kw_in) = _run(tts, REQS, best_of=3, inflight_slots=4, chunk_tokens=8, **KW)
    assert kw_in["slots"] == 4 and "slots" not in kw and tts.gpt.last_inflight["admitted"] == 8        # 12 candidate rows over 4 slots
    assert got == base and sc_in == sc
