"""Per-request logits filters on the device (`itts_gpt_set_row_filters`): `generate(row_filters=)` / `generate(num_beams > 1, group_filters=)`, the
sessions' admissions and `IndexTTS2.infer_requests` with filter kwargs as request keys.  HF has no per-row processors and its rows are
independent, so the expected ids of a mixed batch are ROWS of runs under call-wide filters: the reference's own (tests/golden/gpt_filters_*.npz)
for the f32 greedy cases, the engine's own call-wide runs elsewhere.  Every comparison is bitwise on ids (and on token-score bits where named)."""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as G
from tests.test_gpu_logits_filters import _base_kw, _cfg, _engine, _filter_kw, _ngram_model, _same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STOP = 8193


def _z(golden_dir, name):
    return np.load(os.path.join(golden_dir, f"gpt_{name}.npz"))


def _weights(z):
    cfg = _cfg(z["cfg"])
    sd = G.synth_weights(cfg, seed=int(z["seed"]))
    sd["mel_head.bias"][cfg.stop_mel_token] += float(z["eos_bias"])
    if "one_bias" in z.files:
        sd["mel_head.bias"][1] += float(z["one_bias"])
    return cfg, sd


def _speech(m, z, rows=None, uniforms=None, **kw):
    """`inference_speech` over the fixture's prompts (rows: a list of row indices, default all)"""
    pick = (lambda a: torch.from_numpy(a)) if rows is None else (lambda a: torch.from_numpy(a)[rows])
    codes, _ = m.inference_speech(None, pick(z["text"]), langs=pick(z["langs"]), emo_vec=torch.from_numpy(z["emo_vec"]),
                                  campplus_embedding=torch.from_numpy(z["style"]), max_generate_length=int(z["max_gen"]), uniforms=uniforms, **kw)
    return codes.cpu().numpy()


def _pad(rows, width):
    out = np.full((len(rows), width), STOP, dtype=np.int64)
    for i, r in enumerate(rows):
        assert (r[width:] == STOP).all()
        out[i, :min(width, len(r))] = r[:width]
    return out


# ---- 1. against the reference's own ids ------------------------------------------------------------------------------------------------------
ARRANGEMENTS = {"minlen|minnew4|minnew": ("filters_minlen", "filters_minnew4", "filters_minnew"),
                "none|minnew4|minlen": ("greedy", "filters_minnew4", "filters_minlen")}


@pytest.mark.parametrize("arrangement", list(ARRANGEMENTS))
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("use_graph", [True, False])
def test_mixed_rows_equal_rows_of_the_references_runs(golden_dir, arrangement, compact, use_graph):
    """f32 greedy, three rows with three different entries: row i carries the ids of row i of the reference's generate() under entry i.  With
    compaction at granularity 1 a finished row leaves the batch at once, so a dense row stops being the utterance of the same index: an entry
    read by the dense index would hand the last row another row's min_length."""
    tags = ARRANGEMENTS[arrangement]
    zs = [_z(golden_dir, t) for t in tags]
    base = _z(golden_dir, "greedy")
    cfg, sd = _weights(base)
    m = _engine(cfg, sd)
    m.use_graph = use_graph
    m.set_compaction(compact, 1)
    entries = [None if t == "greedy" else _filter_kw(z) for t, z in zip(tags, zs)]
    want = np.stack([z["codes"][i] for i, z in enumerate(zs)])
    for name in ("greedy", "filters_minnew", "filters_minnew4", "filters_minlen"):       # no single call-wide run gives this batch
        assert not np.array_equal(want, _z(golden_dir, name)["codes"]), name
    got = _speech(m, base, row_filters=entries, **_base_kw(base))
    print(f"{arrangement} graph={use_graph} compact={compact}: lengths {[int((r == STOP).argmax()) for r in got]}")
    _same(got, _pad(want, got.shape[1]), arrangement)
    _same(_speech(m, base, **_base_kw(base)), base["codes"], "plain call afterwards: nothing sticks")


# ---- 2. sampled rows against their scalar runs -----------------------------------------------------------------------------------------------
# Values and a seed at which every entry changes its row's ids on this fixture, in both precisions and both random sources (the test prints
# the first differing step of every row).  min_p 0.3, epsilon 0.08 and eta 0.5 changed their rows under every seed tried; whether the
# n-gram + min_new_tokens entry bites depends on the draw -- measured over the seeds 11, 12, 13 (device stream, and a uniform stream from
# torch's generator under the same seed), only 13 makes it bite in all four cases, at the fixture's temperature 1.0.
SAMPLED_SEED = 13
SAMPLED_ENTRIES = [dict(min_p=0.3), dict(epsilon_cutoff=0.08), dict(eta_cutoff=0.5), dict(no_repeat_ngram_size=2, min_new_tokens=12), None]
SAMPLED_ROWS = [0, 1, 2, 0, 1]


@pytest.mark.parametrize("rng", ["device", "uniforms"])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_sampled_rows_equal_their_call_wide_runs(golden_dir, prec, rng):
    """five sampled rows, one warper / processor each: row i equals row i of the same batch under entry i call-wide"""
    z = _z(golden_dir, "filters_sample_order")
    cfg, sd = _weights(z)
    m = _engine(cfg, sd, prec)
    kw = dict(_base_kw(z), seed=SAMPLED_SEED)
    u = None
    if rng == "uniforms":
        u = torch.rand(int(z["max_gen"]), len(SAMPLED_ROWS), generator=torch.Generator().manual_seed(SAMPLED_SEED), dtype=torch.float64)
    run = lambda **f: _speech(m, z, rows=SAMPLED_ROWS, uniforms=u, **kw, **f)
    width = int(z["max_gen"])
    plain = _pad(run(), width)
    wide = [plain if e is None else _pad(run(**e), width) for e in SAMPLED_ENTRIES]
    got = _pad(run(row_filters=SAMPLED_ENTRIES), width)
    for i, e in enumerate(SAMPLED_ENTRIES):
        diff = np.flatnonzero(wide[i][i] != plain[i])
        print(f"{prec} {rng}: row {i} under {e}: first step that differs from the plain row {diff[:1].tolist()}")
    for i, e in enumerate(SAMPLED_ENTRIES):
        assert np.array_equal(got[i], wide[i][i]), f"row {i} under {e}: {got[i].tolist()} vs call-wide {wide[i][i].tolist()}"
        if e is not None:
            assert not np.array_equal(wide[i][i], plain[i]), f"{e} does not bite on row {i}: the test would pass without the table"
    assert not any(np.array_equal(got, w) for w in wide), "the mixed batch equals one call-wide run as a whole"


# ---- 3. identities ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["minnew", "sample_order"])
def test_the_same_entry_in_every_row_is_the_call_wide_call(golden_dir, tag):
    z = _z(golden_dir, f"filters_{tag}")
    cfg, sd = _weights(z)
    m = _engine(cfg, sd)
    kw = _base_kw(z)
    u = torch.from_numpy(z["uniforms"])[..., 0] if kw["do_sample"] else None
    got = _speech(m, z, uniforms=u, row_filters=[_filter_kw(z)] * 3, **kw)
    _same(got, z["codes"], f"{tag} in every row vs the reference's call-wide ids")
    # ... and the call's own kwargs are the entries' defaults: the call-wide kwargs under a table of empty entries
    _same(_speech(m, z, uniforms=u, row_filters=[None, {}, None], **kw, **_filter_kw(z)), z["codes"], f"{tag} as the call's defaults")


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_a_table_of_off_entries_is_the_plain_call_to_the_bit(golden_dir, prec):
    """ids and, under token_scores=True, the bits of logp_model and logp_sampled"""
    z = _z(golden_dir, "filters_sample_order")
    cfg, sd = _weights(z)
    m = _engine(cfg, sd, prec)
    kw = dict(_base_kw(z), seed=5, token_scores=True)
    off_values = dict(min_new_tokens=0, min_length=0, no_repeat_ngram_size=0, epsilon_cutoff=0.0, eta_cutoff=0.0, suppress_tokens=[])
    runs = []
    for f in ({}, dict(row_filters=[None] * 3), dict(row_filters=[off_values, None, {}])):
        ids = _speech(m, z, **kw, **f)
        ts = m.last_scores
        runs.append((ids, ts.logp_model.cpu().view(torch.int32).numpy(), ts.logp_sampled.cpu().view(torch.int32).numpy()))
    assert (runs[0][1] != 0).any() and (runs[0][2] != 0).any()
    for ids, lm, ls in runs[1:]:
        _same(ids, runs[0][0], "off table vs the plain call")
        assert np.array_equal(lm, runs[0][1]) and np.array_equal(ls, runs[0][2]), "token-score bits differ under a table of off entries"


# ---- 4. one graph serves every rewrite of the table -------------------------------------------------------------------------------------------
def test_one_step_graph_serves_every_table(golden_dir):
    base = _z(golden_dir, "greedy")
    cfg, sd = _weights(base)
    m = _engine(cfg, sd)
    m.use_graph = True
    m.set_compaction(False, 1)                                 # one graph per call shape: a compacted batch replays one per live-row bucket
    kw = _base_kw(base)
    zs = {t: _z(golden_dir, f"filters_{t}") for t in ("minnew", "minnew4", "minlen")}
    _same(_speech(m, base, **kw), base["codes"], "plain call")
    a = _speech(m, base, row_filters=[_filter_kw(zs["minlen"]), _filter_kw(zs["minnew4"]), _filter_kw(zs["minnew"])], **kw)
    cap = m.graph_stats()
    b = _speech(m, base, row_filters=[_filter_kw(zs["minnew"]), None, _filter_kw(zs["minlen"])], **kw)
    _same(_speech(m, base, **kw), base["codes"], "plain call after the mixed ones")
    now = m.graph_stats()
    print(f"graphs captured {cap['captures']} -> {now['captures']}, reused {cap['hits']} -> {now['hits']}")
    assert now["captures"] == cap["captures"] and now["hits"] >= cap["hits"] + 2       # the entries live in device memory, not in the graph
    _same(a, _pad(np.stack([zs["minlen"]["codes"][0], zs["minnew4"]["codes"][1], zs["minnew"]["codes"][2]]), a.shape[1]), "first mixed call")
    _same(b, _pad(np.stack([zs["minnew"]["codes"][0], base["codes"][1], zs["minlen"]["codes"][2]]), b.shape[1]), "second mixed call")


def test_a_grown_table_leaves_no_step_graph_behind_for_the_call_wide_record(golden_dir):
    """One handle, the graph on: a table of two slots, then a table of three (new arrays), then the handle's FIRST call-wide installation, over
    the two rows of the first call.  Were the first table's arrays freed when it grew, the call-wide record could be allocated at their address
    and the step captured under the two-slot table -- which indexes that address by slot -- would be replayed for the call-wide call.  Every
    call is held to rows of the reference's own runs."""
    base = _z(golden_dir, "greedy")
    cfg, sd = _weights(base)
    m = _engine(cfg, sd)
    m.use_graph = True
    m.set_compaction(False, 1)
    kw = _base_kw(base)
    minnew, minlen = _z(golden_dir, "filters_minnew"), _z(golden_dir, "filters_minlen")
    two = _speech(m, base, rows=[1, 2], row_filters=[None, _filter_kw(minlen)], **kw)
    _same(two, _pad(np.stack([base["codes"][1], minlen["codes"][2]]), two.shape[1]), "table of two slots")
    three = _speech(m, base, row_filters=[_filter_kw(minlen), None, _filter_kw(minnew)], **kw)
    _same(three, _pad(np.stack([minlen["codes"][0], base["codes"][1], minnew["codes"][2]]), three.shape[1]), "table of three slots")
    cap = m.graph_stats()["captures"]
    wide = _speech(m, base, rows=[1, 2], **kw, **_filter_kw(minnew))
    _same(wide, _pad(minnew["codes"][1:3], wide.shape[1]), "first call-wide installation after the table grew")
    assert m.graph_stats()["captures"] == cap + 1, "the call-wide call replayed a step captured under a table"
    again = _speech(m, base, rows=[1, 2], row_filters=[None, _filter_kw(minlen)], **kw)      # the larger arrays serve the smaller table again
    _same(again, two, "table of two slots in the grown arrays")


# ---- 5. admission -------------------------------------------------------------------------------------------------------------------------
def test_a_row_admitted_with_its_own_entry_decodes_as_alone_with_it():
    """DecodeSession over a capped row without filters and two rows held past step 30 by entries of their own; at session step 8 a row with
    min_new_tokens, begin_suppress_tokens and no_repeat_ngram_size of its own takes the capped row's slot: it generates what it generates
    alone under these filters call-wide, and the running rows are what they are in the one-shot call without it."""
    from indextts_amd import gpt
    K, AT = 9, 8
    cfg, sd = _ngram_model(4.0)
    m = _engine(cfg, sd)
    g = torch.Generator().manual_seed(152)
    text = torch.randint(2, cfg.number_text_tokens, (3, 9), generator=g)
    text[1, 6:] = 1
    text[2, 8:] = 1
    style, emo = torch.randn(1, 192, generator=g), torch.randn(1, cfg.model_dim, generator=g) * 0.1
    langs = torch.randint(0, cfg.n_langs, (3,), generator=g)
    kw = dict(do_sample=False, num_beams=1, repetition_penalty=1.0)
    prep = lambda t, lg: m.inference_speech_stream(None, t, langs=lg, emo_vec=emo, campplus_embedding=style, max_generate_length=40, **kw)
    emb, mask, mn, hf = prep(text, langs)
    emb_n, mask_n, _, _ = prep(text[1:2, :6].contiguous(), langs[1:2])
    stop = m.stop_mel_token
    ids = lambda row: row[:row.index(stop)] if stop in row else row
    unfiltered = ids(m.generate(emb_n, mask_n, mn, **hf).cpu()[0].tolist())
    entry = dict(min_new_tokens=K, begin_suppress_tokens=[unfiltered[0]], no_repeat_ngram_size=3)
    solo = ids(m.generate(emb_n, mask_n, mn, **hf, **entry).cpu()[0].tolist())
    assert len(solo) >= K and solo[0] != unfiltered[0] and solo != unfiltered
    caps = [4, mn, mn]                                        # slot 0 has ended by step 8, whatever its ids; the others run past step 30
    first = [None, dict(min_new_tokens=30), dict(min_new_tokens=30)]
    running = [ids(r) for r in m.generate(emb, mask, mn, row_max_new=caps, row_filters=first, **hf).cpu().tolist()]
    assert all(len(r) >= 30 for r in running[1:])
    with gpt.DecodeSession(m, emb, mask, mn, row_max_new=caps, row_filters=first, **hf) as s:
        assert s.run(AT) == AT and 0 in s.finished()
        with pytest.raises(ValueError, match="unknown keys"):
            s.admit([0], emb_n, mask_n, row_max_new=[mn], row_filters=[dict(top_k=3)])
        s.admit([0], emb_n, mask_n, row_max_new=[mn], row_filters=[entry])
        while len(s.finished()) < 3 and s.steps < AT + mn:
            s.run(8)
        admitted, others = s.codes(0).cpu().tolist(), [s.codes(b).cpu().tolist() for b in (1, 2)]
    print(f"admitted at session step {AT}: {admitted}; alone {solo}; without filters {unfiltered[:12]}")
    assert admitted == solo
    assert others == running[1:], "the running rows changed"
    assert ids(m.generate(emb_n, mask_n, mn, **hf).cpu()[0].tolist()) == unfiltered       # close() uninstalled the table
    with gpt.DecodeSession(m, emb, mask, mn, row_max_new=caps, **hf) as s:             # a session without a table takes no entries
        s.run(AT)
        with pytest.raises(ValueError, match="row_filters"):
            s.admit([0], emb_n, mask_n, row_max_new=[mn], row_filters=[entry])


# ---- 6. beams -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["beam_sample", "beam_suppress"])
def test_beam_groups_equal_the_scalar_beam_call_with_their_filters(golden_dir, tag):
    """two groups in one 3-beam batch: group 0 beam search under the suppress fixture's kwargs, group 1 beam-sample under the beam-sample
    fixture's -- each the group of the scalar beam call with its own mode and filters call-wide (the draw is keyed by seed, own step, slot)"""
    z = _z(golden_dir, f"filters_{tag}")
    cfg, sd = _weights(z)
    m = _engine(cfg, sd)
    f0, f1 = _filter_kw(_z(golden_dir, "filters_beam_suppress")), _filter_kw(_z(golden_dir, "filters_beam_sample"))
    kw = dict(num_beams=3, top_p=0.95, top_k=8, temperature=1.0, repetition_penalty=10.0, length_penalty=0.0, seed=7)
    width = int(z["max_gen"])
    search = lambda **f: _pad(_speech(m, z, do_sample=False, **kw, **f), width)
    sample = lambda **f: _pad(_speech(m, z, do_sample=True, **kw, **f), width)
    want = np.stack([search(**f0)[0], sample(**f1)[1]])
    plain = np.stack([search()[0], sample()[1]])
    modes = [dict(do_sample=False), dict(do_sample=True)]
    got = _pad(_speech(m, z, do_sample=True, group_sampling=modes, group_filters=[f0, f1], **kw), width)
    print(f"{tag}: lengths under the filters {[int((r == STOP).argmax()) if (r == STOP).any() else width for r in want]}, "
          f"without {[int((r == STOP).argmax()) if (r == STOP).any() else width for r in plain]}")
    assert not np.array_equal(want[0], plain[0]) and not np.array_equal(want[1], plain[1]), "a filter does not bite: the test shows nothing"
    _same(got, want, f"{tag}: groups under their own filters")
    _same(_pad(_speech(m, z, do_sample=True, group_sampling=modes, group_filters=[None, None], **kw), width), plain, "off entries: the plain groups")
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        _speech(m, z, do_sample=True, group_filters=[None, dict(no_repeat_ngram_size=2)], **kw)
    with pytest.raises(ValueError, match="group_filters"):
        _speech(m, z, do_sample=True, row_filters=[None, None], **kw)
    with pytest.raises(ValueError, match="row_filters"):
        _speech(m, z, do_sample=True, group_filters=[None, None], **dict(kw, num_beams=1))


def test_a_beam_group_admitted_with_its_own_entry_ends_as_alone_with_it(golden_dir):
    """BeamDecodeSession over groups without filters: a group admitted with min_new_tokens = K of its own ends with the ids it gets alone"""
    from indextts_amd import gpt
    K = 7
    z, z2 = _z(golden_dir, "beam_sample"), _z(golden_dir, "beam")
    cfg = _cfg(z["cfg"])
    sd = G.synth_weights(cfg, seed=int(z["seed"]))
    sd["mel_head.bias"][cfg.stop_mel_token] += float(z["eos_bias"]) + 1.5
    m = _engine(cfg, sd)
    style, emo = torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"])
    kw = dict(do_sample=False, num_beams=3, repetition_penalty=10.0, length_penalty=1.0)
    prep = lambda t, lg: m.inference_speech_stream(None, t, langs=lg, emo_vec=emo, campplus_embedding=style, max_generate_length=40, **kw)
    emb, mask, mn, hf = prep(torch.from_numpy(z["text"]), torch.from_numpy(z["langs"]))
    emb_n, mask_n, _, _ = prep(torch.from_numpy(z2["text"])[1:2, :6].contiguous(), torch.from_numpy(z2["langs"])[1:2])
    stop = m.stop_mel_token
    ids = lambda row: row[:row.index(stop)] if stop in row else row
    alone = ids(m.generate(emb_n, mask_n, mn, min_new_tokens=K, **hf).cpu()[0].tolist())
    plain = ids(m.generate(emb_n, mask_n, mn, **hf).cpu()[0].tolist())
    assert len(plain) < K <= len(alone)                       # the filter bites on this utterance
    B = emb.shape[0]
    with gpt.BeamDecodeSession(m, emb, mask, mn, group_filters=[None] * B, **hf) as s:
        while not s.finished() and s.steps < mn:
            s.run(4)
        k, slot = s.steps, s.finished()[0]
        with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
            s.admit([slot], emb_n, mask_n, group_filters=[dict(no_repeat_ngram_size=2)])
        s.admit([slot], emb_n, mask_n, group_filters=[dict(min_new_tokens=K)])
        while slot not in s.finished() and s.steps < k + mn:
            s.run(4)
        admitted = s.result(slot).tolist()
    print(f"admitted at session step {k} into slot {slot}: {len(admitted)} ids, alone {len(alone)}, without min_new_tokens {len(plain)}")
    assert admitted == alone


# ---- 7. what a call or session installed leaves with it -------------------------------------------------------------------------------------
_ROUNDS = {}


def _two_rounds(alignment: bool):
    """Twice over, on one engine: (a) a plain greedy generate, (b) one generate with every num_beams = 1 extra installed -- row caps, a
    per-row sampling table, a per-row filter table, token scores, a code prefix and (alignment) the text-attention export --, (c) a
    DecodeSession with the same extras, run(4), close(), (d) the plain greedy generate again.  -> per round the ids of (a), (b), (c), (d)
    and the engine's graph captures after each step.  B = 2, max_new_tokens = 16; only arguments the engine accepts."""
    if alignment in _ROUNDS:
        return _ROUNDS[alignment]
    from indextts_amd import gpt
    cfg, sd = _ngram_model(4.0)
    m = _engine(cfg, sd)
    g = torch.Generator().manual_seed(153)
    text = torch.randint(2, cfg.number_text_tokens, (2, 9), generator=g)
    text[1, 6:] = 1
    style, emo = torch.randn(1, 192, generator=g), torch.randn(1, cfg.model_dim, generator=g) * 0.1
    emb, mask, mn, hf = m.inference_speech_stream(None, text, langs=torch.randint(0, cfg.n_langs, (2,), generator=g), emo_vec=emo,
                                                  campplus_embedding=style, max_generate_length=16, do_sample=False, num_beams=1,
                                                  repetition_penalty=1.0)
    extras = dict(row_max_new=[16, 12], row_sampling=[{}, dict(do_sample=True, top_k=5, seed=3)], row_filters=[None, dict(min_new_tokens=4)],
                  token_scores=True, code_prefix=[[5, 7], None], prefix_chunk=4)
    if alignment:
        extras.update(alignment_heads=[(0, 0), (1, 1)], text_spans=[(3, 8), (3, 6)])
    rounds = []
    for _ in range(2):
        ids, captures = [], []
        for step in "abcd":
            if step in "ad":
                ids.append(m.generate(emb, mask, mn, **hf).cpu())
            elif step == "b":
                ids.append(m.generate(emb, mask, mn, **hf, **extras).cpu())
                assert m.last_scores is not None and m.last_prefix["lens"] == [2, 0] and (m.last_alignment is not None) == alignment
            else:
                s = gpt.DecodeSession(m, emb, mask, mn, **hf, **extras)
                assert s.run(4) == 4
                ids.append(s._codes[:, :6].cpu())                        # (row 0: its two given codes and four of its own)
                s.close()
            captures.append(m.graph_stats()["captures"])
        rounds.append((ids, captures))
    print(f"alignment={alignment}: graph captures after (a), (b), (c), (d): round 1 {rounds[0][1]}, round 2 {rounds[1][1]}")
    _ROUNDS[alignment] = rounds
    return rounds


def test_installed_state_leaves_with_its_call_or_session():
    """the plain greedy ids after a call and a session that installed everything are, to the bit, the ids before them -- in both rounds;
    and the second round's extras decode what the first round's did"""
    (ids1, _), (ids2, _) = _two_rounds(True)
    ids0 = ids1[0]
    assert ids0.shape[0] == 2 and 1 <= ids0.shape[1] <= 16
    for what, got in (("(d), round 1", ids1[3]), ("(a), round 2", ids2[0]), ("(d), round 2", ids2[3])):
        assert torch.equal(got, ids0), f"plain greedy generate {what}: {got.tolist()} vs {ids0.tolist()}"
    assert not torch.equal(ids1[1][:, :ids0.shape[1]], ids0[:, :ids1[1].shape[1]]), "the extras change nothing: the test shows nothing"
    assert ids1[1][0, :2].tolist() == [5, 7] and ids1[2][0, :2].tolist() == [5, 7]          # the full rows, prefix included
    assert torch.equal(ids1[1], ids2[1]) and torch.equal(ids1[2], ids2[2])


@pytest.mark.parametrize("alignment", [True, False], ids=["every_extra", "without_the_alignment_export"])
def test_a_second_round_replays_the_first_rounds_graphs(alignment):
    """the persistent buffers keep their names and shapes, so their addresses -- part of the decode graph's key -- are the first round's and
    the second round of (a) - (d) captures nothing.  With the alignment export that also takes the engine's install epoch (the part of
    the key that stands for the pair list and the sizes a step bakes in) to stay where it is when the same list and sizes are installed
    again: an epoch bumped by every install made (b) and (c) capture once per call, captures [1, 2, 3, 3] then [3, 4, 5, 5]."""
    (_, cap1), (_, cap2) = _two_rounds(alignment)
    assert cap2[-1] == cap1[-1], f"graph captures after (a), (b), (c), (d): round 1 {cap1}, round 2 {cap2}"


# ---- 8. the pipeline ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tts():
    from tests.test_gpu_mixed_requests import VoiceFrontend
    from tests.test_gpu_pipeline import build
    t = build()
    t.frontend = VoiceFrontend(128, device=DEV)
    return t


PIPE_REQUESTS = [dict(spk_audio_prompt="alice.wav", text="hello world", lang="en", seed=11),
                 dict(spk_audio_prompt="bob.wav", text="hello world", lang="en", seed=12),
                 dict(spk_audio_prompt="carol.wav", text="a much longer second sentence here. ok", lang="en", seed=13),
                 dict(spk_audio_prompt="alice.wav", text="one more for the first voice", lang="en", seed=14)]


@pytest.mark.parametrize("mode", [dict(num_beams=1), dict(num_beams=3, beam_settings="own")], ids=["one_beam", "own_beams"])
def test_a_request_with_its_own_filters_gets_what_it_gets_alone(tts, mode):
    """request 0 carries filters of its own (the ids its plain run starts with are suppressed, and a minimum length); in two batches of
    different mates and orders it gets the codes -- bit for bit -- and the waveform it gets alone, where its filters are call-wide"""
    kw = dict(max_mel_tokens=24, **mode)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # (a row may run into its max_mel_tokens)
        tts.infer_requests(PIPE_REQUESTS[:1], **kw)
        plain = tts.last_codes[0].cpu()
        own = dict(PIPE_REQUESTS[0], suppress_tokens=sorted(set(plain[:2].tolist()) - {STOP}), begin_suppress_tokens=[int(plain[2])], min_new_tokens=20)
        (_, w_alone), = tts.infer_requests([own], **kw)
        alone = tts.last_codes[0].cpu()
        alone = alone[: int((alone == STOP).nonzero()[0]) if (alone == STOP).any() else len(alone)]
        assert len(alone) >= 20 and int(alone[0]) != int(plain[0])                     # the filters bite
        mates_alone = {}
        for r in PIPE_REQUESTS[1:]:
            (_, w), = tts.infer_requests([r], **kw)
            mates_alone[r["seed"]] = w
        slots = dict(inflight_slots=2) if mode["num_beams"] == 1 else dict(inflight_beam_slots=2)
        for batch, at, extra in (([own] + PIPE_REQUESTS[1:3], 0, {}), ([PIPE_REQUESTS[3], PIPE_REQUESTS[1], own], 2, {}),
                                 ([PIPE_REQUESTS[3], PIPE_REQUESTS[1], own], 2, slots)):      # ... and admitted into a freed slot of a session
            outs = tts.infer_requests(batch, **kw, **extra)
            codes = tts.last_codes.cpu()
            row = at                                                                   # (one-segment requests come before it)
            assert codes[row, : len(alone)].tolist() == alone.tolist() and (codes[row, len(alone):] == STOP).all(), (codes[row].tolist(), alone.tolist())
            for r, (sr, w) in zip(batch, outs):
                w0 = w_alone if r is own else mates_alone[r["seed"]]
                # the waveform: identical codes through a vocoder batch of another shape -- 1 LSB of int16, the bar of test_gpu_mixed_requests.py
                assert sr == 22050 and w.shape == w0.shape and int(np.abs(w.astype(np.int32) - w0.astype(np.int32)).max()) <= 1
    with pytest.raises(ValueError, match="beam_settings"):
        tts.infer_requests([own, PIPE_REQUESTS[1]], max_mel_tokens=24, num_beams=3)
