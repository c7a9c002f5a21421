"""The GPT decode entries as compositions of shared pieces (`indextts_amd/csrc/capi_gpt.hip`: one call prologue, one step-graph helper, one beam
start, one admission prefill, ONE suspended-loop record).  Engine against engine on a small synthetic model: which entry captures / reuses which
decode-step graph (the graph keys per entry), the captured step against the same step launched plainly, and the suspended-loop record -- a
resume or an admission after ANOTHER call has overwritten the workspace is ITTS_ERR_STATE, a rejected first call leaves the loop resumable."""
import ctypes as C

import pytest
import torch

from oracle import gpt_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_NEW, NB = 12, 3
BEAM = dict(do_sample=False, num_beams=NB, repetition_penalty=10.0, length_penalty=0.0)
GREEDY = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)
CAPS = [MAX_NEW, 2, MAX_NEW]                  # utterance 1 is finished after 2 of its own steps: its slot is the one refilled


@pytest.fixture(scope="module")
def setup():
    """(engine, prep): prep(rows, **generate kwargs) -> (inputs_embeds, attention_mask, max_new, kwargs) of utterances `rows` of four texts"""
    from indextts_amd import gpt
    cfg = G.GPTConfig(layers=2, model_dim=128, heads=2, max_text_tokens=20, max_mel_tokens=40, number_text_tokens=60)
    sd = G.synth_weights(cfg, seed=11)
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, max_text_tokens=cfg.max_text_tokens,
                         max_mel_tokens=cfg.max_mel_tokens, number_text_tokens=cfg.number_text_tokens, precision="fp32", device=DEV)
    m.load_state_dict(sd)
    m.post_init_gpt2_config(kv_cache=True, half=False)
    g = torch.Generator().manual_seed(5)
    text = torch.randint(2, 60, (4, 7), generator=g)
    text[1, 5:] = 1                                               # a shorter text: rows with different left padding
    style, emo = torch.randn(1, 192, generator=g), torch.randn(1, 128, generator=g) * 0.1
    langs = torch.tensor([1, 2, 3, 1])

    def prep(rows, **kw):
        emb, mask, mn, hf = m.inference_speech_stream(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, **kw)
        return emb[rows].contiguous(), mask[rows].contiguous(), mn, hf
    return m, prep


def _delta(m, before):
    s = m.graph_stats()
    return (s["captures"] - before["captures"], s["hits"] - before["hits"])


def _session_with_admission(m, prep, beams: bool):
    """run(4), run(4), admit utterance 3 into the finished slot 1, run(4), run(4) -> ([ids of slot 1 before the admission, ids of every slot at
    the end], graph (captures, hits) of the four run calls)"""
    from indextts_amd import gpt
    kw = BEAM if beams else GREEDY
    emb, mask, mn, hf = prep([0, 1, 2], **kw)
    emb3, mask3, _, _ = prep([3], **kw)
    Session = gpt.BeamDecodeSession if beams else gpt.DecodeSession
    ids_of = (lambda s, b: s.result(b).tolist()) if beams else (lambda s, b: s.codes(b).tolist())
    deltas = []

    def run(s):
        before = m.graph_stats()
        s.run(4)
        deltas.append(_delta(m, before))
    with Session(m, emb, mask, mn, row_max_new=CAPS, **hf) as s:
        run(s)
        run(s)
        assert s.steps == 8 and 1 in s.finished()
        ids = [ids_of(s, 1)]
        s.admit([1], emb3, mask3, row_max_new=[MAX_NEW])
        run(s)
        run(s)
        assert s.steps == 16
        ids += [ids_of(s, b) for b in range(3)]
    return ids, deltas


@pytest.fixture(scope="module")
def sessions(setup):
    """the beam and the row session with an admission, once on the graph path and once on plain launches (shared by the tests below)"""
    m, prep = setup
    out = {}
    try:
        for use_graph in (True, False):
            m.use_graph = use_graph
            for beams in (True, False):
                out[use_graph, beams] = _session_with_admission(m, prep, beams)
    finally:
        m.use_graph = True
    return out


def test_graph_captures_and_hits_per_entry(setup, sessions):
    """One decode-step graph per (entry, key): the one-shot beam call captures once and reuses its graph; a session's key differs from the
    one-shot key (it carries the per-row step table) and changes once with the first admission (the row-shift table)."""
    m, prep = setup
    emb, mask, mn, hf = prep([0, 1, 2], **BEAM)
    before = m.graph_stats()
    a = m.generate(emb, mask, mn, **hf)
    assert _delta(m, before) == (1, 0)
    before = m.graph_stats()
    b = m.generate(emb, mask, mn, **hf)
    assert _delta(m, before) == (0, 1)
    assert torch.equal(a, b)
    for beams in (True, False):
        ids, deltas = sessions[True, beams]
        print(f"{'beam' if beams else 'row'} session: graph (captures, hits) per run {deltas}, lengths {[len(v) for v in ids]}")
        assert deltas == [(1, 0), (0, 1), (1, 0), (0, 1)]
        assert sessions[False, beams][1] == [(0, 0)] * 4


def test_graph_path_equals_plain_launches(sessions):
    """use_graph=False runs the step function handed to the graph helper directly: the ids of a session with an admission are the same"""
    for beams in (True, False):
        graph_ids, plain_ids = sessions[True, beams][0], sessions[False, beams][0]
        assert any(len(v) > 2 for v in graph_ids), graph_ids
        assert graph_ids == plain_ids, f"{'beam' if beams else 'row'} session"


def _raw_calls(m, prep):
    """the four generate entries and the row admission through the C ABI, on ONE workspace: name -> callable(first / args) -> return code"""
    from indextts_amd import _lib, gpt
    L, h, st = _lib.lib(), m._h, _lib.stream_ptr(m.device)
    emb, mask, mn, _ = prep([0, 1, 2])
    x1, pad1, S = m._prefix(emb, mask)
    x3, pad3, _ = m._prefix(emb, mask, NB)
    gp1 = gpt._gen_params(True, mn, 0, repetition_penalty=10.0)
    gp3 = gpt._gen_params(True, mn, 0, num_beams=NB, repetition_penalty=10.0, length_penalty=0.0)
    pen = m._penalty_ids()
    ws = torch.empty(max(L.itts_gpt_workspace_bytes(h, 3, S, S + mn), L.itts_gpt_beam_workspace_bytes(h, 3, NB, S, S + mn)), dtype=torch.uint8, device=DEV)
    adm = torch.empty(L.itts_gpt_admit_workspace_bytes(h, 1, S), dtype=torch.uint8, device=DEV)
    codes = torch.zeros(3, mn, dtype=torch.int64, device=DEV)
    state = m._beam_state(3, NB, mn)
    n = C.c_int32(0)
    p = _lib.ptr

    def rows_chunk(first, limit):
        return L.itts_gpt_generate_chunk(h, p(x1) if first else None, p(pad1), 3, S, C.byref(gp1), pen, 2, None, p(codes), limit, C.byref(n), p(ws),
                                         ws.numel(), 1, st)

    def rows_oneshot():
        return L.itts_gpt_generate(h, p(x1), p(pad1), 3, S, C.byref(gp1), pen, 2, None, p(codes), C.byref(n), p(ws), ws.numel(), 1, st)

    def beam_chunk(first, limit):
        return L.itts_gpt_generate_beam_chunk(h, p(x3) if first else None, p(pad3), 3, NB, S, C.byref(gp3), pen, 2, None, *[p(t) for t in state], limit,
                                              C.byref(n), p(ws), ws.numel(), 1, st)

    def beam_oneshot(num_beams=NB):
        return L.itts_gpt_generate_beam(h, p(x3), p(pad3), 3, num_beams, S, C.byref(gp3), pen, 2, None, *[p(t) for t in state], C.byref(n), p(ws),
                                        ws.numel(), 1, st)

    def admit_row():
        return L.itts_gpt_admit_rows(h, p(x1[:1].contiguous()), p(pad1[:1].contiguous()), (C.c_int32 * 1)(0), 1, S, None, C.byref(gp1), pen, 2, None,
                                     p(codes), p(ws), ws.numel(), p(adm), adm.numel(), st)
    return dict(rows_chunk=rows_chunk, rows_oneshot=rows_oneshot, beam_chunk=beam_chunk, beam_oneshot=beam_oneshot, admit_row=admit_row), codes, state, n


def test_stale_suspended_loop_is_refused(setup):
    """A loop suspended on a workspace that ANOTHER generate call has since overwritten must not be resumed or admitted into: the handle keeps
    one record of what is suspended, and every first call ends it.  (Until the record was one, a one-shot beam call left a suspended row loop
    resumable: the resume decoded from the beam call's cache.)"""
    from indextts_amd import _lib
    m, prep = setup
    call, codes, state, n = _raw_calls(m, prep)
    assert call["rows_chunk"](True, 4) == 0 and n.value == 4
    assert call["beam_oneshot"]() == 0
    torch.cuda.synchronize()
    kept, stats = codes.clone(), m.graph_stats()
    assert call["rows_chunk"](False, 8) == _lib.ERR_STATE, "a row loop whose workspace a beam call has overwritten was resumed"
    assert call["admit_row"]() == _lib.ERR_STATE, "... or admitted into"
    torch.cuda.synchronize()
    assert torch.equal(codes, kept) and m.graph_stats() == stats          # refused before anything was launched
    # the mirror case: a beam loop, then a one-shot row call on its workspace
    assert call["beam_chunk"](True, 4) == 0 and n.value == 4
    assert call["rows_oneshot"]() == 0
    torch.cuda.synchronize()
    kept = [t.clone() for t in state]
    assert call["beam_chunk"](False, 8) == _lib.ERR_STATE
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(state, kept))


def test_rejected_first_call_leaves_the_loop_resumable(setup):
    """a first call ends what is suspended only once its own checks have passed: a row loop outlives a beam call that is an argument error"""
    from indextts_amd import _lib
    m, prep = setup
    call, codes, _, n = _raw_calls(m, prep)
    assert call["rows_chunk"](True, 4) == 0
    assert call["rows_chunk"](False, MAX_NEW) == 0 and n.value == MAX_NEW
    torch.cuda.synchronize()
    want = codes.clone()
    codes.zero_()
    assert call["rows_chunk"](True, 4) == 0
    assert call["beam_oneshot"](num_beams=1) == _lib.ERR_ARG
    assert call["rows_chunk"](False, MAX_NEW) == 0 and n.value == MAX_NEW
    torch.cuda.synchronize()
    assert torch.equal(codes, want) and len(set(want[0].tolist())) > 1
