"""The teacher-forced rescoring pass end to end (`UnifiedVoice.rescore`, `itts_gpt_rescore`) on the tiny synthetic model of the token-score
and alignment tests (3 layers, 2 heads, nine rows over three texts of 10 / 7 / 4 tokens, so three left paddings), and
`IndexTTS2.infer_requests(timestamps="rescore")` on the stub pipeline.

Against the f64 restatement (fp32 engine): tests/align_ref.py's GPT-2 stack, restated here so that it also returns the log-softmax rows, is
run over the prompt and the given ids; the rescored alignment rows -- row 0 included -- and log-probabilities are held to it for greedy
ids, seeded-sampling ids and a 3-beam search's result, with ragged code_lens and chunk 1 / 5 / MAX_NEW.
Against the decode export: for a greedy run with `token_scores=True, alignment_heads=PAIRS`, rows 1 .. L - 1 of the rescored alignment and
all of logp_model agree with the in-step arrays within the sum of the two gates (both sides are within their own gate of the same f64 numbers).
Structure: zeros past code_lens and past the span, identical bits for the same call twice, a suspended `generate_chunks` loop is undisturbed."""
import math

import pytest
import torch

from tests import align_ref as R
from tests import test_gpu_alignment as A
from tests import test_gpu_token_scores as TS
from tests.test_gpu_row_sampling import MAX_NEW, SEED, SETS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = A.PAIRS
N = A.N
CHUNKS = (1, 5, MAX_NEW)
# The restatement gates (test_rescore_equals_the_f64_restatement): 4 x the largest |engine - f64 restatement| observed on the MI355X over the
# test's cases (three id sets x three chunk sizes, nine rows): the alignment weights and the log-probabilities.  The
# margin is for other seeds; the fp32 engine is deterministic.  Either gate above 1e-4 would be a finding to explain, not a tolerance.
ALIGN_OBSERVED = 4.167e-8
LOGP_OBSERVED = 1.791e-6
GATE_ALIGN, GATE_LOGP = 4 * ALIGN_OBSERVED, 4 * LOGP_OBSERVED
assert GATE_ALIGN <= 1e-4 and GATE_LOGP <= 1e-4

_CACHE = {}


def _prompt(golden_dir, prec, rows):
    """(m, emb, mask, x (B, S, D) on the host, pad, spans) of the rows' prompt, as `inference_speech` builds it"""
    m, call, mixed, cfg, sd, text, langs, style, emo, table = A._setup(golden_dir, prec)
    rows = list(rows)
    emb, mask, mn, hf = m.inference_speech_stream(None, text[rows], langs=langs[rows], emo_vec=emo, campplus_embedding=style,
                                                  max_generate_length=MAX_NEW, num_beams=1, alignment_heads=PAIRS)
    x, pad, S = m._prefix(emb, mask)
    return m, emb, mask, x.cpu(), pad.cpu().tolist(), hf["text_spans"]


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def restatement(sd, layers, heads, prefix, pad, ids, pairs, span, pos_offset=2, eps=1e-5):
    """align_ref.teacher_forced_alignment with row 0 and the log-softmax rows: the f64 stack over prefix (S, D) + the decode inputs of ids[:-1];
    the query that predicts code i sits at position S - 1 + i.  -> (attn (n, K, len) f64, logp (n,) f64)"""
    f = lambda name: sd[name].double()
    S, n = prefix.shape[0], len(ids)
    me, mp = f("mel_embedding.weight"), f("mel_pos_embedding.emb.weight")
    rows = [me[int(ids[i - 1])] + mp[i - 1 + pos_offset] for i in range(1, n)]
    x = torch.cat([prefix.double()] + ([torch.stack(rows)] if rows else []), 0)
    T, Dm = x.shape
    dh = Dm // heads
    t = torch.arange(T)
    allowed = (t[None, :] <= t[:, None]) & (t[None, :] >= pad)
    w_of = {}
    for l in range(layers):                                 # align_ref.stack_attention, keeping the residual stream
        p = f"gpt.h.{l}."
        h = R.layer_norm(x, f(p + "ln_1.weight"), f(p + "ln_1.bias"), eps)
        qkv = h @ f(p + "attn.c_attn.weight") + f(p + "attn.c_attn.bias")
        q, k, v = (z.view(T, heads, dh).transpose(0, 1) for z in qkv.split(Dm, dim=1))
        s = q @ k.transpose(1, 2) / math.sqrt(dh)
        w = torch.nan_to_num(torch.softmax(torch.where(allowed[None], s, torch.full((), -math.inf, dtype=torch.float64)), -1), nan=0.0)
        for (pl, ph) in pairs:
            if pl == l:
                w_of[(pl, ph)] = w[ph]
        a = (w @ v).transpose(0, 1).reshape(T, Dm)
        x = x + a @ f(p + "attn.c_proj.weight") + f(p + "attn.c_proj.bias")
        h = R.layer_norm(x, f(p + "ln_2.weight"), f(p + "ln_2.bias"), eps)
        x = x + R.gelu_new(h @ f(p + "mlp.c_fc.weight") + f(p + "mlp.c_fc.bias")) @ f(p + "mlp.c_proj.weight") + f(p + "mlp.c_proj.bias")
    h = R.layer_norm(R.layer_norm(x, f("gpt.ln_f.weight"), f("gpt.ln_f.bias"), eps), f("final_norm.weight"), f("final_norm.bias"), eps)
    logsm = torch.log_softmax(h[S - 1:] @ f("mel_head.weight").t() + f("mel_head.bias"), -1)
    off, ln = span
    attn = torch.zeros(n, len(pairs), ln, dtype=torch.float64)
    for i in range(n):
        for kk, pr in enumerate(pairs):
            attn[i, kk] = w_of[pr][S - 1 + i, pad + off: pad + off + ln]
    return attn, torch.stack([logsm[i, int(ids[i])] for i in range(n)])


def _ids(golden_dir, which):
    """(B, W) ids of the nine-row batch on the host: greedy, seeded sampling, or the result of a 3-beam search"""
    key = ("ids", which)
    if key not in _CACHE:
        m, call, mixed, cfg, sd, text, langs, style, emo, table = A._setup(golden_dir, "fp32")
        if which == "beam":
            ids = m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=3,
                                     do_sample=False, repetition_penalty=10.0, length_penalty=0.0, min_new_tokens=8)[0].cpu()
        else:
            ids, _ = call(range(N), seed=SEED, min_new_tokens=8, **SETS[0 if which == "greedy" else 2])
        _CACHE[key] = ids
    return _CACHE[key]


def _lens(ids, stop):
    """ragged code_lens: every row's own length (up to and including its first stop token), cut by the alignment tests' caps"""
    from indextts_amd import gpt
    own, _ = gpt.TokenScores.lengths_of(ids, [ids.shape[1]] * ids.shape[0], stop)
    return [min(int(o), c) for o, c in zip(own.tolist(), A.CAPS)]


def _reference(golden_dir, which):
    key = ("ref", which)
    if key not in _CACHE:
        m, emb, mask, x, pad, spans = _prompt(golden_dir, "fp32", range(N))
        _, _, _, cfg, sd, *_ = A._setup(golden_dir, "fp32")
        ids = _ids(golden_dir, which)
        lens = _lens(ids, m.stop_mel_token)
        _CACHE[key] = (lens, [restatement(sd, cfg.layers, cfg.heads, x[b], pad[b], ids[b, :lens[b]].tolist(), PAIRS, spans[b]) for b in range(N)])
    return _CACHE[key]


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("which", ["greedy", "sampled", "beam"])
def test_rescore_equals_the_f64_restatement(golden_dir, which, chunk):
    m, emb, mask, x, pad, spans = _prompt(golden_dir, "fp32", range(N))
    ids = _ids(golden_dir, which)
    lens, ref = _reference(golden_dir, which)
    assert len(set(pad)) == 3 and len(set(lens)) >= 4 and min(lens) >= 4, (pad, lens)
    ts, al = m.rescore(emb, mask, ids.to(DEV), code_lens=lens, alignment_heads=PAIRS, text_spans=spans, chunk=chunk)
    assert ts.logp_sampled is None and ts.lengths.tolist() == lens == al.lengths.tolist()
    attn, logp = al.attn.cpu().double(), ts.logp_model.cpu().double()
    worst_a = worst_l = 0.0
    for b in range(N):
        L, T = lens[b], spans[b][1]
        want_a, want_l = ref[b]
        worst_a = max(worst_a, float((attn[b, :L, :, :T] - want_a).abs().max()))
        worst_l = max(worst_l, float((logp[b, :L] - want_l).abs().max()))
        assert float(want_a.sum(-1).min()) > 1e-3, "the span must carry attention mass in every row (row 0 too), or the comparison shows nothing"
        assert float((want_a[:, 0] - want_a[:, 1]).abs().max()) > 10 * GATE_ALIGN and float(want_l.min()) < -1e-2
        # structure: nothing past code_lens, nothing past the span
        assert bool((attn[b, L:] == 0).all()) and bool((logp[b, L:] == 0).all()) and bool((attn[b, :, :, T:] == 0).all()), f"row {b}"
    print(f"{which} chunk {chunk}: lens {lens}; max |engine - f64| alignment {worst_a:.3e} (gate {GATE_ALIGN:.3e}), logp {worst_l:.3e} (gate {GATE_LOGP:.3e})")
    assert worst_a <= GATE_ALIGN and worst_l <= GATE_LOGP


def test_rescore_agrees_with_the_decode_export(golden_dir):
    m, call, mixed, cfg, sd, text, langs, style, emo, table = A._setup(golden_dir, "fp32")
    rows = list(range(N))                                   # the nine-row batch: three left paddings
    ids, al = call(rows, seed=SEED, token_scores=True, alignment_heads=PAIRS, min_new_tokens=8, **SETS[0])
    dec_lm, dec_len = m.last_scores.logp_model.cpu(), m.last_scores.lengths.tolist()
    _, emb, mask, x, pad, spans = _prompt(golden_dir, "fp32", rows)
    assert len(set(pad)) == 3, pad
    ts, ra = m.rescore(emb, mask, ids.to(DEV), alignment_heads=PAIRS, text_spans=spans)          # code_lens=None: up to the first stop token
    assert ts.lengths.tolist() == dec_len == al.lengths.tolist()
    gate_a, gate_l = A.GATE + GATE_ALIGN, TS.GATE + GATE_LOGP
    equal_a = equal_l = True
    worst_a = worst_l = 0.0
    for b in range(len(rows)):
        L, T = dec_len[b], spans[b][1]
        assert L >= 4
        da = (ra.attn[b, 1:L, :, :T].cpu().double() - al.attn[b, 1:L, :, :T].double()).abs().max()
        dl = (ts.logp_model[b, :L].cpu().double() - dec_lm[b, :L].double()).abs().max()
        worst_a, worst_l = max(worst_a, float(da)), max(worst_l, float(dl))
        assert float(da) <= gate_a and float(dl) <= gate_l, (b, float(da), float(dl))
        assert bool((al.attn[b, 0] == 0).all()) and float(ra.attn[b, 0, :, :T].sum()) > 1e-3, "row 0: zero in the decode export, written by the rescoring pass"
        equal_a &= _bits(ra.attn[b, 1:L, :, :T].cpu(), al.attn[b, 1:L, :, :T])
        equal_l &= _bits(ts.logp_model[b, :L].cpu(), dec_lm[b, :L])
    print(f"rescored vs in-step (fp32, greedy): alignment rows bit-equal: {equal_a}; logp_model bit-equal: {equal_l}; "
          f"max |d| alignment {worst_a:.3e} (gate {gate_a:.3e}), logp {worst_l:.3e} (gate {gate_l:.3e})")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_structure_repeatability_and_chunking(golden_dir, prec):
    m, emb, mask, x, pad, spans = _prompt(golden_dir, prec, range(N))
    ids = _ids(golden_dir, "sampled")
    lens = _lens(ids, m.stop_mel_token)
    lens[4] = 0                                             # a row with nothing to score: all zeros
    runs = {}
    for chunk in CHUNKS:
        ts, al = m.rescore(emb, mask, ids.to(DEV), code_lens=lens, alignment_heads=PAIRS, text_spans=spans, chunk=chunk)
        ts2, al2 = m.rescore(emb, mask, ids.to(DEV), code_lens=lens, alignment_heads=PAIRS, text_spans=spans, chunk=chunk)
        assert _bits(ts.logp_model.cpu(), ts2.logp_model.cpu()) and _bits(al.attn.cpu(), al2.attn.cpu()), f"chunk {chunk}: the same call twice"
        runs[chunk] = (ts.logp_model.cpu(), al.attn.cpu())
        lp, at = runs[chunk]
        assert at.shape == (N, ids.shape[1], len(PAIRS), max(4, (max(l for _, l in spans) + 3) // 4 * 4)) and lp.shape == tuple(ids.shape)
        for b in range(N):
            L, T = lens[b], spans[b][1]
            assert bool((lp[b, L:] == 0).all()) and bool((at[b, L:] == 0).all()) and bool((at[b, :, :, T:] == 0).all()), f"row {b}"
            assert bool(torch.isfinite(lp[b, :L]).all()) and bool((lp[b, :L] < 0).all()) and bool((at[b, :L] >= 0).all())
            s = at[b, :L, :, :T].sum(-1)
            assert L == 0 or (bool((s > 0).all()) and float(s.max()) <= 1 + 1e-6), f"row {b}"
    if prec == "fp32":                                      # chunked and one-shot results agree within the gate (the gates are the fp32 engine's:
        for chunk in CHUNKS[:-1]:                           # the bf16 half of this test holds structure and repeatability only)
            dl = float((runs[chunk][0].double() - runs[MAX_NEW][0].double()).abs().max())
            da = float((runs[chunk][1].double() - runs[MAX_NEW][1].double()).abs().max())
            print(f"chunk {chunk} vs one-shot: max |d| logp {dl:.3e} (gate {GATE_LOGP:.3e}), alignment {da:.3e} (gate {GATE_ALIGN:.3e})")
            assert dl <= GATE_LOGP and da <= GATE_ALIGN
    # an absurd shape is refused by the workspace query (0) before anything is formed from it
    from indextts_amd import _lib
    wsb = _lib.lib().itts_gpt_rescore_workspace_bytes
    assert wsb(m._h, N, 20, MAX_NEW, 5) > 0
    assert wsb(m._h, 65536, 20, MAX_NEW, 5) == 0 and wsb(m._h, 40000, 20, 65535, 65535) == 0 and wsb(m._h, 40000, 65535, MAX_NEW, 5) == 0
    # scores alone: no heads, the same log-probabilities
    ts3, none = m.rescore(emb, mask, ids.to(DEV), code_lens=lens, chunk=5)
    assert none is None and m.last_alignment is None and _bits(ts3.logp_model.cpu(), runs[5][0])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_suspended_generate_chunks_loop_continues_unchanged(golden_dir, prec):
    m, call, mixed, cfg, sd, text, langs, style, emo, table = A._setup(golden_dir, prec)
    rows = [0, 1, 2, 3]
    emb, mask, mn, hf = m.inference_speech_stream(None, text[rows], langs=langs[rows], emo_vec=emo, campplus_embedding=style,
                                                  max_generate_length=MAX_NEW, do_sample=False, num_beams=1, seed=SEED, min_new_tokens=20)
    kw = dict(hf)
    kw.pop("uniforms", None)
    plain = [c[0].cpu() for c in m.generate_chunks(emb, mask, mn, 8, 2, **kw)]
    assert len(plain) >= 3, "the loop must be suspended more than once, or the test shows nothing"
    _, emb9, mask9, x, pad, spans = _prompt(golden_dir, prec, range(N))
    ids9 = _ids(golden_dir, "greedy")
    got = []
    for c in m.generate_chunks(emb, mask, mn, 8, 2, **kw):
        got.append(c[0].cpu())
        m.rescore(emb9, mask9, ids9.to(DEV), alignment_heads=PAIRS, text_spans=spans, chunk=5)       # between two chunk calls of the loop
    assert len(got) == len(plain) and all(torch.equal(a, b) for a, b in zip(got, plain)), "the suspended loop's ids changed"


# ---- the pipeline ------------------------------------------------------------------------------------------------------------------------
tts = A.tts
HEADS = [(1, 0), (0, 1)]
SHARED = [dict(spk_audio_prompt=r["spk_audio_prompt"], text=r["text"], lang="en") for r in A.REQS]


@pytest.mark.filterwarnings("ignore:WARN. generation stopped:RuntimeWarning")
@pytest.mark.parametrize("mode", ["shared", "own"])
def test_pipeline_timestamps_are_segment_timestamps_of_the_rescored_last_codes(tts, mode):
    from indextts_amd.infer_v2_5 import IndexTTS2
    reqs = SHARED if mode == "shared" else A.REQS
    kw = dict(num_beams=3, max_mel_tokens=24, interval_silence=100, seed=5) if mode == "shared" else \
        dict(num_beams=3, beam_settings="own", max_mel_tokens=24, interval_silence=100)
    torch.manual_seed(3)
    plain = tts.infer_requests(reqs, **kw)
    codes_plain = tts.last_codes.clone()
    assert tts.last_timestamps is None and tts.last_scores is None
    rescore_calls, ts_calls = [], []
    real_rescore = tts.gpt.inference_speech_rescore

    def rec_rescore(*a, **k):
        out = real_rescore(*a, **k)
        rescore_calls.append((a, k, out))
        return out

    def rec_ts(*a):
        out = IndexTTS2.segment_timestamps(*a)
        ts_calls.append((a, out))
        return out
    tts.gpt.inference_speech_rescore, tts.segment_timestamps = rec_rescore, rec_ts
    try:
        torch.manual_seed(3)
        outs = tts.infer_requests(reqs, timestamps="rescore", alignment_heads=HEADS, **kw)
    finally:
        del tts.gpt.inference_speech_rescore, tts.segment_timestamps
    # codes and audio are those of the call without the kwarg
    assert torch.equal(tts.last_codes, codes_plain)
    assert all(a[0] == b[0] and a[1].shape == b[1].shape and (a[1] == b[1]).all() for a, b in zip(outs, plain))
    # ONE batched pass over last_codes ...
    (a, k, (rs, ra)), = rescore_calls
    assert torch.equal(a[2], tts.last_codes) and a[2].shape[0] == 4 and k["alignment_heads"] == HEADS
    rs2, ra2 = real_rescore(*a, **k)
    assert _bits(ra2.attn.cpu(), ra.attn.cpu()) and _bits(rs2.logp_model.cpu(), rs.logp_model.cpu())
    # ... and the timestamps are exactly segment_timestamps of its paths
    assert len(ts_calls) == 4
    _, code_lens = tts.trim_codes(tts.last_codes)
    for i, (args, out) in enumerate(ts_calls):
        n_codes = int(code_lens[i])
        assert args[2] == n_codes and torch.equal(torch.as_tensor(args[0]), ra2.row(i).path(0, "mean", n_codes=n_codes))
    assert tts.last_timestamps == [[ts_calls[0][1]], [ts_calls[1][1], ts_calls[2][1]], [ts_calls[3][1]]]
    for r, (sr, w) in enumerate(outs):
        flat = [e for seg in tts.last_timestamps[r] for e in seg]
        assert flat and flat[0]["start"] == 0.0 and abs(flat[-1]["end"] - w.shape[0] / 22050.0) < 1e-9
        assert all(x["start"] <= x["end"] for x in flat) and all(x["end"] <= y["start"] + 1e-12 for x, y in zip(flat, flat[1:]))
    sc = tts.last_scores
    assert [len(r) for r in sc] == [1, 2, 1] and all(s["mean_logprob"] < 0 and s["lengths"] >= 1 for r in sc for s in r)
    assert [s["mean_logprob"] for r in sc for s in r] == rs2.mean_logprob().tolist()
    # timestamps=True keeps its refusal in the same call
    with pytest.raises(ValueError, match="num_beams"):
        tts.infer_requests(reqs, timestamps=True, alignment_heads=HEADS, **kw)
    # num_beams = 1 is allowed: the second pass replaces the in-step export
    tts.infer_requests(A.REQS, num_beams=1, max_mel_tokens=24, timestamps="rescore", alignment_heads=HEADS, interval_silence=100)
    assert [len(t) for t in tts.last_timestamps] == [1, 2, 1]
