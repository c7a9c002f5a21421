"""What tests/select_matrix.py rests on, checked on the CPU (tests/test_gpu_select_matrix.py then holds the kernels to the table):

* the constant-logits model puts the row in front of the selection, bit for bit, in the f32 and in the bf16 arithmetic contract;
* the oracle's new `tie_rule="index"` changes nothing where nothing ties: the ids of the unchanged oracle on every tie-free case and on the
  committed `gpt_*.npz` goldens under their own settings;
* the restatement of the selection (`select_matrix.restate`) gives the oracle's ids on every case the oracle can state;
* the margin gate: the restatement in f64 -- the high-precision reference here: the oracle itself casts its logits to f32 -- gives the f32
  ids, and every comparison it makes is an exact tie (|a - b| = 0 in f64: the same row value, the same beam-score bits) or is decided by
  1e-4 (scores, cumulative probabilities) / 1e-9 (u * total against the CDF steps); beam cases also keep their ids when every distinct row
  value's log-probability moves by an ulp (another correct log_softmax), so no sum of three that merely equals another in exact arithmetic
  decides.  No case is exempt but the one that IS a sub-ulp comparison, the top-p threshold finding, which has a test of its own;
* every named defect of `select_matrix.DEFECTS` changes the ids of at least one case;
* every branch of the beam scorer the table means to reach is reached."""
import os

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as G
from tests import select_matrix as M
from tests.test_oracle_gpt import gen_params as golden_gen_params, load_case

CASES = M.cases()
IDS = [c.name for c in CASES]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


_EXPECTED = {}


def _restated(case):
    """the f32 restatement's ids, computed once per case and left unchanged"""
    if case.name not in _EXPECTED:
        _EXPECTED[case.name] = M.restate(case)
    return _EXPECTED[case.name]


def test_the_table_covers_the_sizes_paths_and_families():
    for V in M.SIZES:
        fam = {c.family for c in CASES if c.V == V}
        assert {"greedy", "sample"} <= fam, (V, fam)
    for V in (257, 8194):
        assert any(c.radix == (0, 1) and c.family == "sample" for c in CASES if c.V == V), f"both top-k paths at {V}"
    assert {int(c.st["num_beams"]) for c in CASES if c.family == "beam"} == {2, 3, 4}
    assert {float(dict(c.st, **r).get("length_penalty")) for c in CASES if c.family == "beam" for r in (c.rows or [{}])} == {0.0, 1.0, 2.0}
    assert any(c.family == "beam" and any(dict(c.st, **r).get("do_sample") for r in (c.rows or [{}])) for c in CASES)
    assert all(c.max_new <= 16 and c.B <= 4 for c in CASES)


@pytest.mark.parametrize("V", M.SIZES)
def test_the_head_returns_the_row_whatever_the_hidden_state(V):
    """zero weight, bias = row: `lm_head` of any finite hidden state is the row, in both arithmetic contracts (0 * h sums to an exact 0)"""
    cfg = M.config(V)
    rows = {c.row.numpy().tobytes(): c.row for c in CASES if c.V == V}
    h = torch.randn(2, 3, cfg.model_dim, generator=torch.Generator().manual_seed(V)) * 30.0
    for row in rows.values():
        sd = M.weights(V, row)
        for mode in ("f32", "bf16"):
            with G.numerics(mode):
                out = G.lm_head(G.bf16_weights(sd) if mode == "bf16" else sd, cfg, h)
            assert torch.equal(out, row.expand_as(out)), mode


@pytest.mark.parametrize("case", [c for c in CASES if c.family != "beam"], ids=[c.name for c in CASES if c.family != "beam"])
def test_the_oracle_sees_the_row_at_every_step(case):
    """the logits trace of `generate_sample` (every step, every row of the case) equals the row"""
    trace = []
    M.oracle_ids(case, trace=trace)
    assert len(trace) == case.B
    for tr in trace:
        assert len(tr["logits"]) >= 1
        for lg in tr["logits"]:
            assert lg.dtype == torch.float32 and torch.equal(lg[0], case.row)


@pytest.mark.parametrize("case", [c for c in CASES if not c.ties], ids=[c.name for c in CASES if not c.ties])
def test_the_tie_rule_changes_nothing_on_a_tie_free_case(case):
    assert not case.cap and not case.engine_thr
    assert _same(M.oracle_ids(case, tie_rule=None), M.oracle_ids(case, tie_rule="index"))


def test_the_tie_rule_matters_on_the_cases_that_say_so():
    """the unchanged oracle (torch.sort without `stable`, torch.topk) gives other ids on some of the tie cases: the rule is not vacuous"""
    differ = [c.name for c in CASES if c.ties and not c.cap and not c.engine_thr and not _same(M.oracle_ids(c, tie_rule=None), M.oracle_ids(c))]
    print(f"{len(differ)} tie cases on which the reference's calls give other ids: {differ}")
    assert any(n.startswith("top-p-0.75-on-8-equal") for n in differ) and any(n.startswith("beam") for n in differ)


@pytest.mark.parametrize("tag", ["greedy", "greedy_nokv", "sample", "beam", "beam_sample", "greedy_mid", "typical_sample", "typical_greedy",
                                 "typical_beam_sample"])
def test_the_tie_rule_leaves_the_goldens_alone(golden_dir, tag):
    """tests/test_oracle_gpt.py::test_codes_match_reference under `tie_rule="index"`: the reference's own ids, so the fixture model never ties"""
    z, cfg, sd = load_case(golden_dir, tag)
    gp = golden_gen_params(z)
    gp.tie_rule = "index"
    u = torch.from_numpy(z["uniforms"])
    if gp.num_beams == 1:
        u = u[..., 0]
    conds = G.conds_latent_campplus(sd, torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"]))
    with torch.no_grad():
        codes = G.inference_speech(sd, cfg, conds, torch.from_numpy(z["text"]), torch.from_numpy(z["langs"]), gp, uniforms=u,
                                   kv_cache=bool(z["kv_cache"]))
    assert np.array_equal(codes.numpy(), z["codes"])


def test_the_oracle_refuses_an_unknown_tie_rule():
    with pytest.raises(AssertionError):
        G.process_scores(torch.zeros(1, 8), torch.zeros(1, 1, dtype=torch.long), G.GenParams(tie_rule="value"))


@pytest.mark.parametrize("case", [c for c in CASES if not (c.cap or c.engine_thr)], ids=[c.name for c in CASES if not (c.cap or c.engine_thr)])
def test_the_restatement_gives_the_oracles_ids(case):
    assert _same(_restated(case), M.oracle_ids(case)), (_restated(case).tolist(), M.oracle_ids(case).tolist())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_margin_gate(case):
    log = M.Log()
    ids64 = M.restate(case, torch.float64, log=log)
    assert _same(ids64, _restated(case)), f"f64 gives {ids64.tolist()}, f32 {_restated(case).tolist()}"
    near = log.near()
    if case.gate:
        assert not near, f"decided by less than the gate's margin: {near[:8]}"
    else:
        assert case.engine_thr and all(k == "cum" and m < 1e-7 for k, m in near), near      # the threshold finding: sub-ulp by construction
    if case.family == "beam":
        for seed in range(8):
            assert _same(M.run_beam(case, jitter=seed), _restated(case)), f"an ulp on the log-probabilities (seed {seed}) changes the ids"
    if case.walk is not None:
        assert set(M.expected_ids(case).flatten().tolist()) == set(case.walk), "the draws do not cover the kept set"


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_every_named_defect_changes_some_case(defect):
    killed = []
    for c in CASES:
        try:
            ids = M.restate(c, defect=defect)
        except AssertionError:                             # (the restated scorer ran out of non-stop candidates: not the table's ids either)
            killed.append(c.name)
            continue
        if not _same(ids, _restated(c)):
            killed.append(c.name)
    print(f"{defect}: changes {len(killed)} cases: {killed[:6]}")
    assert killed, f"no case notices: {defect}"


def test_every_branch_of_the_beam_scorer_is_reached():
    log = M.Log()
    for c in CASES:
        if c.family == "beam":
            M.run_beam(c, log=log)
    want = {"step 0: every candidate from beam 0", "a stop candidate of rank < nb became a hypothesis", "a stop candidate of rank >= nb was passed over",
            "the heap filled", "a better hypothesis replaced the worst", "a hypothesis no better than the worst was dropped", "the done rule fired",
            "the done rule did not fire on a full heap", "open beams finalised at max_length", "the best hypotheses differ in length: padded output"}
    assert want <= log.events, want - log.events
    assert "step 0: a dead beam survived" not in log.events


@pytest.mark.parametrize("name", [c.name for c in CASES if c.engine_thr])
def test_the_top_p_threshold_finding(name):
    """top_p = 0.8 on five equal scores.  Each has probability 0.2f.  The reference compares the cumulative sum with `1 - top_p` formed in
    double and rounded once, 0.2f: `<=` removes one score, 4 stay.  The engine forms `1 - top_p` from the f32 top_p, 0.19999999f, one ulp
    below: nothing is removed, 5 stay (DESIGN: the documented threshold; the table asserts it in this one case)."""
    case = M.by_name(name)
    five = sorted(case.walk)
    ref = M.oracle_ids(case)
    assert set(ref.flatten().tolist()) == set(five[1:]), "the reference keeps the four of higher index"
    eng = M.restate(case)
    assert set(eng.flatten().tolist()) == set(five), "the engine's threshold keeps all five"
    assert _same(M.restate(case._replace(engine_thr=False)), ref), "the restatement under the reference's threshold is the oracle"
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
    assert f32(1.0 - 0.8) == f32(0.2) and f32(1.0 - f32(0.8)) < f32(0.2)
    # where the complement is exact in f32 the two thresholds are one number: no other case depends on which is used
    for c in CASES:
        if not c.engine_thr and c.family != "beam":
            assert _same(M.restate(c._replace(engine_thr=True)), _restated(c)), c.name


@pytest.mark.parametrize("case", [c for c in CASES if c.cap], ids=[c.name for c in CASES if c.cap])
def test_the_cap_rule(case):
    """more ties on the k-th value than survivor slots: the reference keeps them all (the restatement without a cap is the oracle); the engine's
    rule keeps the scores above the threshold and the tied ones of lowest index, 128 in all, and the draws show the difference"""
    assert _same(M.restate(case._replace(cap=False)), M.oracle_ids(case))
    assert not _same(_restated(case), M.oracle_ids(case))
    x = case.row
    kth = float(torch.sort(x, descending=True)[0][int(case.st["top_k"]) - 1])
    above, tied = torch.nonzero(x > kth).flatten(), torch.nonzero(x == kth).flatten()
    kept = set(above.tolist()) | set(tied[: M.SAMPLE_CAP - above.numel()].tolist())
    assert tied.numel() + above.numel() > M.SAMPLE_CAP and set(_restated(case).flatten().tolist()) <= kept
    assert int(_restated(case)[0, -1]) == max(kept), "u next to 1 draws the last kept id: the tied score of 125th-lowest index or a higher one"
    assert int(_restated(case)[0, -2]) == min(kept)


def test_the_beam_cap_case_needs_no_rule_of_its_own():
    """100 scores tie on the maximum, 64 slots: with the lowest indices kept the top 2 nb are the oracle's, cap or no cap"""
    for c in CASES:
        if c.name.startswith("beam3-more-ties-than-slots"):
            assert int((c.row == c.row.max()).sum()) > M.BEAM_CAP
            assert _same(M.run_beam(c._replace(cap=True)), M.oracle_ids(c))
