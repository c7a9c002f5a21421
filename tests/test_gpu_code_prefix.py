"""Continue generation from a given code prefix (`generate(code_prefix=)`, `inference_speech(input_tokens=)`, `itts_gpt_set_code_prefix`) on the
tiny fixtures of the token-score and alignment tests (3 layers, D = 128, MAX_NEW = 40).

Against the CPU oracle (fp32, the given uniform stream; expected ids come from tests/code_prefix_ref.py and oracle.gpt_oracle, never from the
engine): the resume rule returns the oracle's plain rows whole, a foreign prefix continues as the decode-rule restatement says, the reference
rule equals the unchanged oracle on cat(fake ids, prefix).  Every compared case first asserts, from the oracle's trace, that its smallest
decision margin is at least code_prefix_ref.MIN_MARGIN (100 x the largest engine-vs-f64 score difference on record): the many-query ingest is
not bit-equal to decoded steps, and a decision closer than that would compare rounding, not rules.
Structure (fp32 and bf16, each compared with itself only): a row's full ids do not depend on its batch mates, its slot or the other rows'
prefix lengths, with and without compaction; `generate`, `generate_chunks` and an admission into a `DecodeSession` agree; repeat calls are
bit-identical, scores included; no stale step graph; an installed table makes the beam entry fail."""
import warnings

import numpy as np
import pytest
import torch

from tests import code_prefix_ref as R
from tests.test_gpu_alignment import CAPS, N
from tests.test_gpu_alignment import _setup as _nine_setup
from tests.test_gpu_row_sampling import MAX_NEW, SEED, SETS, _scalar_kw
from tests.test_gpu_token_scores import GATE
from tests.test_gpu_token_scores import _setup as _scores_setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
assert MAX_NEW == R.MAX_NEW and SETS == R.SETS


def _engine_call(golden_dir):
    m, call, *_ = _scores_setup(golden_dir, "fp32")
    return m, call


def _assert_margin(trace, new_ids, s, uniforms, stop, what):
    margin = R.decision_margin(trace, new_ids, s, uniforms, stop)
    print(f"{what}: smallest decision margin {margin:.3e} (needs {R.MIN_MARGIN:.3e})")
    assert margin >= R.MIN_MARGIN, f"{what}: margin {margin:.3e} below {R.MIN_MARGIN:.3e}: replace the case"


# ---- 1. resume equals the plain run ------------------------------------------------------------------------------------------------------
# two ragged length vectors, clipped to each row's plain length - 1: with prefix_chunk 1 / 5 / 64 the first gives k = chunk - 1, chunk (chunk 1),
# one pass (chunk 64) and whole passes; the second gives k = chunk - 1, chunk, chunk + 1 at chunk 5 and, with 11 codes, a last pass of one
@pytest.mark.parametrize("si", [0, 1, 2, 3])
def test_resume_returns_the_oracles_plain_rows(golden_dir, si):
    fx = R.fixture(golden_dir)
    m, call = _engine_call(golden_dir)
    s, plain, stop = SETS[si], fx["plain"][si], fx["stop"]
    _assert_margin(fx["traces"][si], plain, s, fx["uniforms"], stop, f"set {si} plain run")
    n = [R.n_codes(r, stop) for r in plain]
    lens_own = [min(n[b] + 1, plain.shape[1]) for b in range(4)]              # codes and the stop token
    for want, chunks in (([0, 1, 7, None], (1, 5, 64)), ([4, 5, 6, 11], (5,))):
        ks = [min(n[b] - 1, n[b] - 1 if w is None else w) for b, w in enumerate(want)]
        assert all(0 <= k < MAX_NEW for k in ks)
        for chunk in chunks:
            got, _ = call(uniforms=fx["uniforms"], seed=SEED, code_prefix=[plain[b, :k] for b, k in enumerate(ks)], prefix_chunk=chunk,
                          **_scalar_kw(s))
            lp = m.last_prefix
            assert lp is not None and lp["lens"] == ks, "the call must record that the ingest ran"
            # (the engine also clamps a pass to the prompt bucket, so that the ingest fits the decode workspace: never fewer passes than this)
            assert lp["chunks"] >= (-(-max(ks) // min(chunk, max(ks))) if max(ks) else 0) and (lp["chunks"] > 0) == (max(ks) > 0)
            if chunk <= 5:
                assert lp["chunks"] == -(-max(ks) // min(chunk, max(ks)))
            assert torch.equal(got, plain), f"set {si} k {ks} chunk {chunk}: {got.tolist()} vs the oracle's plain rows {plain.tolist()}"
            assert lp["decode_steps"] <= max(l - k for l, k in zip(lens_own, ks)) + 8, (lp, lens_own, ks)
    again, _ = call(uniforms=fx["uniforms"], seed=SEED, **_scalar_kw(s))
    assert m.last_prefix is None and torch.equal(again, plain), "a call without a prefix leaves last_prefix = None and the plain ids"


# ---- 2. foreign prefix -------------------------------------------------------------------------------------------------------------------
# (continuing set, the set whose run gives the prefix, k); margins computed on the CPU oracle when the cases were chosen: 3.8e-3, 1.6e-3,
# 8.5e-4 (sampled), 2.5e-4 (sampled, typical)
FOREIGN = [(0, 3, 5), (1, 2, 3), (2, 0, 5), (3, 0, 5)]


@pytest.mark.parametrize("si,sj,k", FOREIGN)
def test_foreign_prefix_continues_as_the_decode_rule_says(golden_dir, si, sj, k):
    fx = R.fixture(golden_dir)
    m, call = _engine_call(golden_dir)
    s, stop = SETS[si], fx["stop"]
    prefix = fx["plain"][sj][:, :k]
    assert not bool((prefix == stop).any())
    tr = {}
    new = R.continue_run(fx, s, prefix, "resume", tr)
    _assert_margin(tr, new, s, fx["uniforms"][k:], stop, f"set {si} after {k} codes of set {sj}")
    want = torch.cat([prefix, new], dim=1)
    plain = fx["plain"][si]
    w = min(want.shape[1], plain.shape[1])
    assert all(not torch.equal(want[b, :w], plain[b, :w]) for b in range(4)), "the expected rows must differ from the plain run"
    got, _ = call(uniforms=fx["uniforms"], seed=SEED, code_prefix=prefix, prefix_chunk=4, **_scalar_kw(s))
    assert m.last_prefix["lens"] == [k] * 4
    assert torch.equal(got, want), f"{got.tolist()} vs {want.tolist()}"


# ---- 3. the reference rule against the unchanged oracle -----------------------------------------------------------------------------------
# margins computed on the CPU oracle: sets 0 / 1 at k = 1, 4, 13: 1.6e-2, 6.2e-3, 1.1e-2; set 2 at k = 1, 4: 1.9e-4, 5.1e-4; set 3 at k = 1,
# 13: 1.2e-3, 6.0e-4 (set 3 at k = 4 decides at 7.4e-5 and is left out)
REFERENCE = [(0, 1), (0, 4), (0, 13), (1, 1), (1, 4), (1, 13), (2, 1), (2, 4), (3, 1), (3, 13)]


@pytest.mark.parametrize("si,k", REFERENCE)
def test_input_tokens_equal_the_unchanged_oracle(golden_dir, si, k):
    fx = R.fixture(golden_dir)
    m, _ = _engine_call(golden_dir)
    s, stop, plain = SETS[si], fx["stop"], fx["plain"][si]
    prefix = plain[:, :k]
    assert not bool((prefix == stop).any())
    tr = {}
    want = R.continue_run(fx, s, prefix, "reference", tr)
    _assert_margin(tr, want, s, fx["uniforms"][k:], stop, f"set {si} input_tokens of {k}")
    tail = plain[:, k:]
    w = min(want.shape[1], tail.shape[1])
    assert any(not torch.equal(want[b, :w], tail[b, :w]) for b in range(4)), "the reference rule must differ from the plain tail"
    got = m.inference_speech(None, fx["text"], langs=fx["langs"], emo_vec=fx["emo"], campplus_embedding=fx["style"], max_generate_length=MAX_NEW - k,
                             num_beams=1, input_tokens=prefix, uniforms=fx["uniforms"], seed=SEED, **_scalar_kw(s))[0].cpu()
    assert m.last_prefix["lens"] == [k] * 4
    assert torch.equal(got, want), f"{got.tolist()} vs {want.tolist()}"
    one = m.inference_speech(None, fx["text"][:1], langs=fx["langs"][:1], emo_vec=fx["emo"], campplus_embedding=fx["style"],
                             max_generate_length=MAX_NEW - k, num_beams=1, input_tokens=prefix[0], uniforms=fx["uniforms"][:, :1], seed=SEED,
                             **_scalar_kw(s))[0].cpu()                         # the (s,) form
    n0 = R.n_codes(want[0], stop) + 1
    assert torch.equal(one[0, :n0], want[0, :n0])


# ---- 4. scores -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [0, 2, 3])
def test_scores_of_the_continued_columns_against_the_oracle_trace(golden_dir, si):
    """logp_model / logp_sampled of the continued columns against the f64 log_softmax of the plain run's trace (the continuation IS the plain
    run's tail, test 1), at test_gpu_token_scores.GATE; prefix columns hold 0.0 and the means skip them.  Observed maxima on the MI355X are
    recorded in DESIGN section 18."""
    fx = R.fixture(golden_dir)
    m, call = _engine_call(golden_dir)
    s, plain, stop, tr = SETS[si], fx["plain"][si], fx["stop"], fx["traces"][si]
    n = [R.n_codes(r, stop) for r in plain]
    ks = [0, min(1, n[1] - 1), min(7, n[2] - 1), n[3] - 1]
    ids, ts = call(uniforms=fx["uniforms"], seed=SEED, token_scores=True, code_prefix=[plain[b, :k] for b, k in enumerate(ks)], prefix_chunk=5,
                   **_scalar_kw(s))
    ts = m.last_scores
    assert torch.equal(ids, plain) and ts.starts.tolist() == ks
    d_model, d_sampled = [], []
    for b in range(4):
        L = int(ts.lengths[b])
        assert L == min(n[b] + 1, MAX_NEW), (b, L, n[b])
        assert bool((ts.logp_model[b, :ks[b]] == 0).all()) and bool((ts.logp_sampled[b, :ks[b]] == 0).all()), f"row {b}: a prefix column is scored"
        for t in range(ks[b], L):
            tok = int(ids[b, t])
            d_model.append(abs(float(ts.logp_model[b, t]) - float(torch.log_softmax(tr["logits"][t][b].double(), -1)[tok])))
            d_sampled.append(abs(float(ts.logp_sampled[b, t]) - float(torch.log_softmax(tr["scores"][t][b].double(), -1)[tok])))
    print(f"set {si} k {ks}: {len(d_model)} continued entries, max |logp_model - oracle| {max(d_model):.3e}, max |logp_sampled - oracle| "
          f"{max(d_sampled):.3e} (gate {GATE:.3e})")
    assert len(d_model) >= 20
    assert max(d_model) <= GATE and max(d_sampled) <= GATE
    want = [float(ts.logp_model[b, ks[b]:int(ts.lengths[b])].double().mean()) for b in range(4)]
    assert ts.mean_logprob().tolist() == pytest.approx(want, abs=1e-12)


# ---- 5. structure ---------------------------------------------------------------------------------------------------------------------------
_PLAIN = {}                                    # per precision: the nine rows' plain runs alone (computed once, never modified) and prefix lengths


def _prefixes(golden_dir, prec):
    """nine rows (three left paddings, their own settings and caps): each row's plain run alone, and a prefix of it of 0 / 1 / 2 / .. codes"""
    m, call, mixed, *_ = _nine_setup(golden_dir, prec)
    if prec not in _PLAIN:
        plain = [mixed([i])[0][0] for i in range(N)]
        lens = []
        for i, row in enumerate(plain):
            n = R.n_codes(row, m.stop_mel_token)
            lens.append(max(0, min([0, 1, 2, 3, 5, 6, 7, 9, 4][i], n - 1, CAPS[i] - 1)))
        _PLAIN[prec] = (plain, lens)
    plain, lens = _PLAIN[prec]
    return m, mixed, [plain[i][:lens[i]] for i in range(N)], lens


def _full_rows(ids, stop):
    return [r[: R.n_codes(r, stop) + 1].clone() for r in ids]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("compaction", [False, True])
def test_a_rows_ids_do_not_depend_on_its_batch_mates(golden_dir, prec, compaction):
    m, mixed, pre, lens = _prefixes(golden_dir, prec)
    stop = m.stop_mel_token
    assert len(set(lens)) >= 5 and max(lens) >= 5, lens
    alone = [_full_rows(mixed([i], code_prefix=[pre[i]])[0], stop)[0] for i in range(N)]
    for i in range(N):
        assert torch.equal(alone[i][:lens[i]], pre[i]), "the returned row starts with its prefix"
    m.set_compaction(compaction, 1)
    try:
        order = list(range(N))
        got = _full_rows(mixed(order, code_prefix=[pre[i] for i in order])[0], stop)
        stats = dict(m.last_timing)
        rev = order[::-1]                                          # other slots; and with rows 0 .. 3 bare, other prefix lengths around each row
        got_rev = _full_rows(mixed(rev, code_prefix=[pre[i] if i > 3 else None for i in rev])[0], stop)
    finally:
        m.set_compaction(True, 8)
    assert stats["compactions"] >= 1 if compaction else stats["compactions"] == 0
    for i in range(N):
        assert torch.equal(got[i], alone[i]), f"{prec} row {i}: {got[i].tolist()} vs alone {alone[i].tolist()}"
        if i > 3:
            assert torch.equal(got_rev[N - 1 - i], alone[i]), f"{prec} row {i} in slot {N - 1 - i}"
    print(f"{prec} compaction={compaction}: prefix lengths {lens}, full lengths {[int(r.numel()) for r in got]}, compactions {stats['compactions']}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_generate_chunks_and_an_admission_agree_with_generate(golden_dir, prec):
    from indextts_amd import gpt
    m, call, mixed, cfg, sd, text, langs, style, emo, table = _nine_setup(golden_dir, prec)
    _, _, pre, lens = _prefixes(golden_dir, prec)
    stop = m.stop_mel_token
    rows = [3, 5, 7, 8]                                            # prefix lengths 3, 6, 9, 4 (where the rows allow them)
    tab = [table[i] for i in rows]
    want = _full_rows(call(rows, row_sampling=tab, do_sample=False, seed=SEED, code_prefix=[pre[i] for i in rows], prefix_chunk=4)[0], stop)
    emb, mask, mn, hf = m.inference_speech_stream(None, text[rows], langs=langs[rows], emo_vec=emo, campplus_embedding=style,
                                                  max_generate_length=MAX_NEW, do_sample=False, num_beams=1, seed=SEED)
    hf.pop("uniforms", None)
    # generate_chunks: chunks of 8 codes without overlap, stitched by their lengths
    parts = [[] for _ in rows]
    for chunk, last, done, clens in m.generate_chunks(emb, mask, mn, 8, 0, row_sampling=tab, code_prefix=[pre[i] for i in rows], prefix_chunk=4, **hf):
        for b in range(len(rows)):
            parts[b].append(chunk[b, : int(clens[b])].cpu())
    assert m.last_prefix is not None and m.last_prefix["lens"] == [lens[i] for i in rows]
    for b, i in enumerate(rows):
        got = torch.cat(parts[b])
        assert torch.equal(got, want[b][: R.n_codes(want[b], stop)]), f"{prec} generate_chunks row {i}: {got.tolist()} vs {want[b].tolist()}"
    # a session whose first batch brings prefixes, and admissions with a prefix at step 8 and past MAX_NEW
    own, S2, new = dict(table[7], stream=0, seed=4321), 4321, 7
    solo = _full_rows(call([new], row_sampling=[own], do_sample=False, seed=SEED, row_max_new=[MAX_NEW], code_prefix=[pre[new]],
                           prefix_chunk=4)[0], stop)[0]
    caps = [MAX_NEW, 7, 25, 17]
    admitted_at = []
    with gpt.DecodeSession(m, emb, mask, mn, row_sampling=tab, row_max_new=caps, code_prefix=[pre[i] for i in rows], prefix_chunk=4, **hf) as s:
        s.run(8)
        assert m.last_prefix["lens"] == [lens[i] for i in rows]
        for at_least in (8, MAX_NEW + 9):
            while s.steps < at_least or not s.finished():
                s.run(8)
            slot = s.finished()[0]
            if at_least == 8:                                      # the first occupants: full rows, prefix included, cut at their caps
                for b, i in enumerate(rows):
                    if b in s.finished():
                        assert torch.equal(s.codes(b).cpu(), want[b][: min(R.n_codes(want[b], stop), caps[b])]), f"{prec} first batch slot {b}"
            k = s.steps
            s.admit([slot], emb[2:3], mask[2:3], row_max_new=[MAX_NEW], row_sampling=[own], code_prefix=[pre[new]])
            assert m.last_prefix["lens"] == [lens[new]]
            while slot not in s.finished() and s.steps < k + 2 * MAX_NEW:
                s.run(8)
            assert torch.equal(s.codes(slot).cpu(), solo[: R.n_codes(solo, stop)]), f"{prec} admitted at step {k}: {s.codes(slot).tolist()} vs {solo.tolist()}"
            admitted_at.append(k)
    assert admitted_at[0] < MAX_NEW < admitted_at[1]
    print(f"{prec}: prefix lengths {[lens[i] for i in rows]} / admitted {lens[new]} at steps {admitted_at}")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_repeat_calls_widths_and_the_plain_call(golden_dir, prec):
    """the same call twice is bit-identical, scores included; another prefix width, and no prefix, between two equal calls never replays a
    stale step graph"""
    m, call, mixed, *_ = _nine_setup(golden_dir, prec)
    _, _, pre, lens = _prefixes(golden_dir, prec)
    rows = [4, 5, 6, 7]
    bits = lambda a, b: a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))

    def run(prefix):
        ids, _ = mixed(rows, token_scores=True, **({} if prefix is None else dict(code_prefix=prefix)))
        ts = m.last_scores
        return ids, ts.logp_model.cpu(), ts.logp_sampled.cpu(), ts.lengths.tolist()
    plain = run(None)
    a = run([pre[i] for i in rows])
    b = run([pre[i] for i in rows])
    short = run([pre[i][:2] for i in rows])                        # another table width
    plain2 = run(None)
    c = run([pre[i] for i in rows])
    for x in (b, c):
        assert torch.equal(x[0], a[0]) and bits(x[1], a[1]) and bits(x[2], a[2]) and x[3] == a[3]
    assert torch.equal(plain2[0], plain[0]) and bits(plain2[1], plain[1]) and bits(plain2[2], plain[2])
    for r, i in enumerate(rows):
        assert torch.equal(a[0][r, :lens[i]], pre[i]) and torch.equal(short[0][r, :min(2, lens[i])], pre[i][:2])
        assert bool((a[1][r, :lens[i]] == 0).all())


def test_an_installed_table_makes_the_beam_entry_fail(golden_dir):
    from indextts_amd import _lib
    m, call, mixed, cfg, sd, text, langs, style, emo, table = _nine_setup(golden_dir, "fp32")
    prefix = (torch.tensor([[5, 6, 7]] * 2, device=DEV), [3, 2])
    m._install_prefix(prefix, 128)
    try:
        with pytest.raises(_lib.HipEngineError, match="code prefix"):
            m.inference_speech(None, text[:2], langs=langs[:2], emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=3,
                               do_sample=False)
        with pytest.raises(_lib.HipEngineError, match="rows"):      # a table of 2 rows does not serve a batch of 3
            m.inference_speech(None, text[:3], langs=langs[:3], emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=1,
                               do_sample=False)
    finally:
        m._uninstall_prefix()
    with pytest.raises(NotImplementedError, match="num_beams"):
        m.inference_speech(None, text[:2], langs=langs[:2], emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=3,
                           do_sample=False, code_prefix=[[5, 6], None])
    ids = m.inference_speech(None, text[:2], langs=langs[:2], emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=3,
                             do_sample=False)[0]
    assert ids.shape[0] == 2                                       # uninstalled: the beam entry runs again


# ---- 6. pipeline ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tts():
    from tests.test_gpu_pipeline import build
    return build()


REQS = [dict(spk_audio_prompt="a.wav", text="hello world. a much longer second sentence here", lang="en", seed=11, temperature=0.9),
        dict(spk_audio_prompt="b.wav", text="and one more", lang="en", seed=12, top_k=8),
        dict(spk_audio_prompt="a.wav", text="the last of them", lang="en", seed=13)]


def test_pipeline_requests_resume_in_any_slot_and_through_inflight_slots(tts):
    kw = dict(num_beams=1, max_mel_tokens=24)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        outs = tts.infer_requests(REQS, **kw)
        full = tts.last_codes.cpu().clone()                        # rows: request 0's two segments, request 1, request 2
        stop = int(tts.stop_mel_token)
        n = [R.n_codes(r, stop) for r in full]
        assert min(n) >= 3, n
        cut = [n[0] // 2, None, 2, n[3] - 1]                       # per row; row 1 (request 0's second segment) starts from nothing
        pre = [None if c is None else full[i, :c].tolist() for i, c in enumerate(cut)]
        reqs = [dict(REQS[0], code_prefix=[pre[0], pre[1]]), dict(REQS[1], code_prefix=pre[2]), dict(REQS[2], code_prefix=[pre[3]])]
        again = tts.infer_requests(reqs, **kw)
        assert tts.gpt.last_prefix is not None and tts.gpt.last_prefix["lens"] == [c or 0 for c in cut]
        got = tts.last_codes.cpu()
        for i in range(4):
            assert torch.equal(got[i, : n[i] + 1], full[i, : n[i] + 1]), f"row {i}: {got[i].tolist()} vs uninterrupted {full[i].tolist()}"
        for (sr, w), (sr0, w0) in zip(again, outs):                # the audio renders the full codes
            assert w.shape == w0.shape and int(np.abs(w.astype(np.int32) - w0.astype(np.int32)).max()) <= 1
        # another order (other slots), and through two in-flight slots
        for extra in (dict(), dict(inflight_slots=2)):
            tts.infer_requests(reqs[::-1], **kw, **extra)
            rev = tts.last_codes.cpu()
            for i, j in ((0, 2), (1, 3), (2, 1), (3, 0)):          # rows of the reversed call: request 2, request 1, request 0's two segments
                assert torch.equal(rev[j, : n[i] + 1], full[i, : n[i] + 1]), f"{extra} row {i}"
            if extra:
                assert tts.gpt.last_inflight["admitted"] >= 1
        # a foreign seed continues the same prefix somewhere else, and still starts with it
        tts.infer_requests([dict(reqs[1], seed=99)], **kw)
        assert tts.last_codes.cpu()[0, :2].tolist() == pre[2]
        # best_of: every candidate shares the prefix; candidate 0 draws from the request's own stream, so it is the resume
        tts.infer_requests([dict(reqs[1], best_of=3)], **kw)
        report, winner = tts.last_scores[0][0], tts.last_codes.cpu()[0]
        assert len(report["mean_logprob"]) == 3 and tts.gpt.last_prefix["lens"] == [2, 2, 2]
        assert winner[:2].tolist() == pre[2]
        assert report["lengths"][0] == min(n[2] + 1, 24), "candidate 0 is the resume: the uninterrupted row's length, prefix counted"
        if report["chosen"] == 0:
            assert torch.equal(winner[: n[2] + 1], full[2, : n[2] + 1])
        with pytest.raises(ValueError, match="rescore"):
            tts.infer_requests(reqs, timestamps=True, alignment_heads=[(0, 0)], **kw)
        with pytest.raises(NotImplementedError, match="num_beams"):
            tts.infer_requests(reqs, max_mel_tokens=24)
