"""CPU: the premises of the vocoder test matrix (tests/voc_matrix.py) that tests/test_gpu_voc_matrix.py relies on -- the path list is the
library's, every path has cases and the edges named in the matrix are present, the exact operands are exact, the f64 references notice the
defects the GPU comparison is there to catch, and the bounds sit where a correct f32 evaluation passes with room while today's unit tolerance
is not loosened.  No device: the library loads without one."""
import collections
import threading

import pytest
import torch
import torch.nn.functional as F

from tests import voc_matrix as VM

SHAPES = list({VM._shape_key(c): c for c in VM.CONV_CASES}.values())        # one case per distinct operand set


def test_path_list_is_the_library_s():
    from indextts_amd import _lib
    assert _lib.voc_path_names() == VM.ALL_PATHS
    assert _lib.lib().itts_voc_path_name(len(VM.ALL_PATHS)) is None and _lib.lib().itts_voc_path_name(-1) is None
    seen = []
    t = threading.Thread(target=lambda: seen.append(_lib.voc_last_path()))       # the record is per thread: a new one has launched nothing
    t.start()
    t.join()
    assert seen == ["none"]


def test_every_path_has_cases_and_ids_are_unique():
    n = collections.Counter([c.path for c in VM.CONV_CASES] + [c.path for c in VM.ACT_CASES])
    assert [p for p in VM.ALL_PATHS if n[p] < 10] == []
    assert set(n) == set(VM.ALL_PATHS)
    ids = [VM.conv_id(c) for c in VM.CONV_CASES] + [VM.act_id(c) for c in VM.ACT_CASES]
    assert len(set(ids)) == len(ids)
    assert 250 <= len(VM.CONV_CASES) <= 400 and 100 <= len(VM.ACT_CASES) <= 140
    for c in VM.CONV_CASES:                                    # the size limits that keep a case well under a second
        assert c.Cin <= 96 and c.Cout <= 384 and c.T <= 1030 and c.epi in VM.EPILOGUES[c.op] + ("full",)
    for c in VM.ACT_CASES:
        assert c.T <= 2050


def _has(pred, cases=VM.CONV_CASES):
    return any(pred(c) for c in cases)


def test_conv_edges_are_present():
    f32 = lambda bm: [c for c in VM.CONV_CASES if c.op == "f32" and c.path == f"conv_f32_bm{bm}"]
    for bm in (32, 64, 96, 128):
        cs = f32(bm)
        assert {c.T for c in cs} >= set(VM.F32_T_BM128 if bm == 128 else VM.F32_T), bm
        assert {c.Cout for c in cs} >= set(VM.F32_COUT[bm]), bm
        assert {c.Cin for c in cs} >= set(VM.F32_CIN), bm
        assert {(c.k, c.d) for c in cs} >= set(VM.F32_KD), bm
        assert {c.epi for c in cs if c.lens is None} >= set(VM.EPILOGUES["f32"]), bm
        ft = VM.F32_FRAME_TILE[bm]
        for nco in (1, 3):                                     # XCD slot mapping: B * n_frame_tiles, with one and with three channel tiles
            got = {c.B * -(-c.T // ft) for c in cs if -(-c.Cout // bm) == nco and c.lens is None}
            assert got >= set(VM.XCD_TILES), (bm, nco, got)
        assert _has(lambda c: c.lens is not None and c.lm == 1, cs) and _has(lambda c: c.lm == 2, cs), bm
    assert max((c.k - 1) * c.d for c in VM.CONV_CASES if c.op in ("f32", "x3")) == VM.CONV_HALO       # exactly the halo
    for bm in (32, 128):
        cs = [c for c in VM.CONV_CASES if c.op == "convT" and c.path == f"conv_f32_bm{bm}"]
        assert {(c.k, c.d) for c in cs} >= set(VM.CONVT_KU) and {c.T for c in cs} >= set(VM.CONVT_TIN), bm
        assert {c.epi for c in cs} >= set(VM.EPILOGUES["convT"]) and _has(lambda c: c.lens is not None and c.lm == 1, cs) and _has(lambda c: c.lm == 2, cs)
        assert {dict(c.opts)["conv_bm"] for c in cs} == {0 if bm == 32 else 128}
    x3 = [c for c in VM.CONV_CASES if c.op == "x3"]
    assert {c.T for c in x3} >= set(VM.X3_T) and {c.Cout for c in x3} >= set(VM.X3_COUT) and {c.Cin for c in x3} >= set(VM.X3_CIN)
    assert {(c.k, c.d) for c in x3} >= set(VM.X3_KD)
    assert all((c.path == "conv_x3_nh2") == (c.Cout > 96) for c in x3)
    two = [c for c in VM.CONV_CASES if c.path == "conv_h3_two_stage"]
    assert {c.T for c in two} >= set(VM.H3_TWO_T) and {c.Cout for c in two} >= set(VM.H3_TWO_COUT)
    assert _has(lambda c: c.k == 1, two) and _has(lambda c: (c.k - 1) * c.d > 48 and not c.opts, two) and _has(lambda c: dict(c.opts).get("h3_kernel") == 0, two)
    for path, (couts, ts) in VM.H3_WIN.items():
        cs = [c for c in VM.CONV_CASES if c.path == path]
        assert {c.Cout for c in cs} >= set(couts) and {c.T for c in cs} >= set(ts), path
        assert max((c.k - 1) * c.d for c in cs) == 48, path
    for c in VM.CONV_CASES:
        if c.op == "h3":
            assert VM.h3_path(c.Cout, c.k, c.d, dict(c.opts).get("h3_kernel", 1)) == c.path, VM.conv_id(c)
    for op in ("f32", "x3", "h3", "convT"):                    # every mode: ragged rows with 0, 1, T and above T; len_mult 2; every epilogue
        cs = [c for c in VM.CONV_CASES if c.op == op]
        assert _has(lambda c: c.lens is not None and c.lm == 1 and {0, 1, c.T} <= set(c.lens) and max(c.lens) > c.T, cs), op
        assert _has(lambda c: c.lm == 2 and 0 in c.lens, cs), op
        assert {c.epi for c in cs} >= set(VM.EPILOGUES[op]), op


def test_activation_edges_are_present():
    for path in VM.ACT_PATHS:
        cs = [c for c in VM.ACT_CASES if c.path == path]
        assert {c.T for c in cs} == set(VM.ACT_T) and {c.C for c in cs} == set(VM.ACT_C[path]), path
        for pset in ("mild", "wide"):
            assert {c.logscale for c in cs if c.pset == pset} == {0, 1}, (path, pset)
            assert {c.T for c in cs if c.pset == pset} == set(VM.ACT_T), (path, pset)
        tile = VM.ACT_TILE[path]
        rag = [c for c in cs if c.lens is not None and c.lm == 1]
        assert any({0, 1, tile - 1, tile + 1} <= set(c.lens) and max(c.lens) > c.T for c in rag), path
        assert any(c.lm == 2 for c in cs), path


def test_exact_operands_are_exact():
    for c in SHAPES:
        o = VM.operands(c, "exact")
        for t in o[:6]:
            assert torch.equal(t * 4, (t * 4).round())                                   # multiples of 1/4
            assert torch.equal(t.bfloat16().float(), t) and torch.equal(t.half().float(), t)
        assert float(o.x.abs().max()) <= 8 and float(o.w.abs().max()) <= 2 and o.div == 4.0
        assert max(float(t.abs().max()) for t in o[2:6]) <= 16
        for split in (VM.split_h3(o.x)[1], VM.split_h3(o.w)[1], *VM.split_x3(o.x)[1:], *VM.split_x3(o.w)[1:]):
            assert not bool(split.any())                                                 # the low parts / planes are zero
        assert 16 * VM.n_terms(c) + 48 < 2 ** 24                                         # reach of any partial sum, in units of 1/4: * 4 still far below
    # the density of zeros differs per input channel, per output channel and per tap
    c = next(c for c in SHAPES if c.op == "f32" and c.Cin == 40 and c.k == 7)
    o = VM.operands(c, "exact")
    z = (o.w == 0).double()
    assert z.mean((1, 2)).std() > 0.03 and z.mean((0, 2)).std() > 0.03 and z.mean((0, 1)).std() > 0.03
    assert (o.x == 0).double().mean((0, 2)).std() > 0.1


@pytest.mark.parametrize("op", ["f32", "x3", "h3", "convT"])
def test_integer_convolutions_notice_defects(op):
    c = next(c for c in VM.CONV_CASES if c.op == op and c.k >= 3 and c.epi == "bias" and c.lens is None and c.T >= 100)
    o = VM.operands(c, "exact")
    ref = VM.ref64(c, o)
    for j in range(c.k):
        assert not torch.equal(VM.ref64(c, o, drop_tap=j), ref), f"dropped tap {j}"
        assert not torch.equal(VM.ref64(c, o, shift_tap=j), ref), f"tap {j} one frame off"
    x2 = o.x.clone()
    x2[:, [0, 1]] = o.x[:, [1, 0]]
    assert not torch.equal(VM.ref64(c, o._replace(x=x2)), ref), "swapped input channel pair"
    perm = list(range(c.Cout))
    perm[0], perm[1] = 1, 0
    w2 = o.w[:, perm] if op == "convT" else o.w[perm]
    assert not torch.equal(VM.ref64(c, o._replace(w=w2)), ref), "swapped output channel pair"
    assert not torch.equal(VM.ref64(c, o._replace(bias=torch.zeros_like(o.bias))), ref), "dropped bias"
    # and any f32 evaluation of these operands is exact
    assert torch.equal(VM.seq32(c, o).double(), ref) and torch.equal(VM.seq32(c, o, reverse=True).double(), ref)


def _torch_f32(c, o):
    x = VM.zero_beyond(c, o.x)
    if c.op == "convT":
        return F.conv_transpose1d(x, o.w, stride=c.d, padding=(c.k - c.d) // 2)
    return F.conv1d(x, o.w, dilation=c.d, padding=(c.k - 1) // 2 * c.d)


def test_f32_evaluations_sit_at_half_the_bound_and_split_emulations_inside_their_terms():
    worst = collections.defaultdict(float)
    for c in VM.CONV_CASES:
        o = VM.operands(c, "wide")
        ref, bd, m = VM.ref64(c, o), VM.bound(c, o), VM.valid_mask(c)
        if not bool(m.any()):
            continue
        r = lambda y: float(((y.double() - ref).abs() / bd)[m].max())
        worst["seq32"] = max(worst["seq32"], r(VM.seq32(c, o)))
        worst["torch"] = max(worst["torch"], r(VM.epilogue(c, _torch_f32(c, o), o, torch.float32)))
        if c.op in ("x3", "h3"):
            term = VM.split_term(c, o) / (o.div if VM.flags(c)[3] == 2 else 1.0)
            worst[c.op] = max(worst[c.op], float(((VM.split_emulation(c, o) - ref).abs() / term)[m].max()))
    print(dict(worst))
    assert worst["seq32"] <= 0.5 and worst["torch"] <= 0.5, dict(worst)
    assert 0 < worst["x3"] <= 1.0 and 0 < worst["h3"] <= 1.0, dict(worst)


def test_rms_criterion_covers_two_thirds_of_every_conv_path_and_notices_a_lost_plane():
    for p in VM.CONV_PATHS:
        cs = [c for c in VM.CONV_CASES if c.path == p]
        share = sum(VM.carries_rms(c) for c in cs) / len(cs)
        assert share >= 2 / 3, (p, share)
    # two opposite summation orders of the f32 baseline stay inside the margin of each other (the channel scales are log-normal, so the order
    # decides which products meet a large partial sum); a kernel that lost its lowest plane / part does not pass
    for op in ("x3", "h3"):
        c = next(c for c in VM.CONV_CASES if c.op == op and c.Cin == 96 and c.k == 11)
        o = VM.operands(c, "wide")
        ref, m = VM.ref64(c, o), VM.valid_mask(c)
        a, b = VM.rms(VM.seq32(c, o).double() - ref, m), VM.rms(VM.seq32(c, o, reverse=True).double() - ref, m)
        assert max(a, b) / min(a, b) < VM.RMS_MARGIN, (a, b)
        x = VM.zero_beyond(c, o.x)
        if op == "x3":
            xh, xm, _ = VM.split_x3(x)
            lost = xh.double() + xm.double()
        else:
            lost = VM.split_h3(x)[0]
        y = VM.epilogue(c, VM.conv_lin(c, lost, o.w.double()), o, torch.float64)
        assert VM.rms(y - ref, m) > VM.rms_limit(c, o, ref), op


def test_activation_bound_is_not_looser_than_the_unit_tolerance_and_f32_passes_with_room():
    assert VM.E_VSIN == 2 * VM.E_VSIN_MEASURED and VM.E_VSIN <= VM.E_VSIN_CAP
    worst = collections.defaultdict(float)
    for c in VM.ACT_CASES:
        ref, bd, m = VM.act_ref_bound(c)
        if not bool(m.any()):
            continue
        if c.pset == "mild":
            assert float(bd[m].max()) < 2e-5 * max(1.0, float(ref[m].abs().max())), VM.act_id(c)
        worst[c.pset] = max(worst[c.pset], float(((VM.act_f32(c).double() - ref).abs() / bd)[m].max()))
    print(dict(worst))
    assert worst["mild"] <= 0.5 and worst["wide"] <= 0.5, dict(worst)
    # the wide set is what it is there for: arguments of thousands of radians, a gain above 10
    big = [c for c in VM.ACT_CASES if c.pset == "wide" and c.T >= 1023]
    assert max(float((VM.act_operands(c).x.abs().max() * (VM.act_operands(c).alpha.exp() if c.logscale else VM.act_operands(c).alpha).max())) for c in big) > 1000
    assert max(float((1 / (VM.act_operands(c).beta.exp() if c.logscale else VM.act_operands(c).beta)).max()) for c in big) > 10


def test_probe_points():
    g = VM.probe_grid()
    assert g.numel() >= 2 ** 20 + 5 * 129 - 1 and float(g.abs().max()) <= 3.1416 + 1e-4
    for v in (0.0, 1.5707964, -1.5707964, 3.1415927, -3.1415927):
        assert bool((g == torch.tensor(v)).any())
    r = VM.probe_range()
    assert float(r.abs().min()) <= 2.0 ** -30 and float(r.abs().max()) >= 2.0 ** 20
    assert float(VM.probe_bound(torch.tensor([0.0])).item()) == VM.E_VSIN + 2.0 ** -22
