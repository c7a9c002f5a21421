"""CPU: the premises of tests/test_gpu_attn_matrix.py, checked without a device -- the f64 reference is the definition (a brute-force
loop agrees), the one-hot operands really give the target's V row bitwise, the uniform sums are exact, the bf16 operands are bf16 values,
every table index is in range, the matrix names every kernel path -- and the matrix can fail: a reference with one deliberate defect
(a window edge off by one either way, an interior key dropped at a chunk or wrap boundary, the wrong row-map parity, an ignored seq_map
or pos_shift, swapped heads) does not pass the comparisons the GPU file applies, in any case the defect applies to."""
import collections
import math

import pytest
import torch

from tests import attn_matrix as AM

BY = collections.Counter()          # (mutant, family that caught it) -> cases


def _brute(c, q, k, v):
    """The definition as a loop over (sequence, head, query), written without the module's geometry code."""
    out = torch.zeros(c.nseq, c.nq, AM.D, dtype=torch.float64)
    m0, m1 = AM.row_maps(c.nseq, c.Tmax)
    for b in range(c.nseq):
        pb = c.seq_map[b] if c.seq_map is not None else b * max(c.seq_mul, 1)
        first = c.pad[pb] if c.pad is not None else 0
        for qi in range(c.nq):
            last = min(c.pos + qi - (c.shift[pb] if c.shift is not None else 0), c.Tmax - 1)
            for h in range(AM.H):
                ts = list(range(first, last + 1))
                if not ts:
                    continue
                row = [int((m1 if c.step & 1 else m0)[b, t]) if c.rmap else pb for t in ts]
                qv = q[b, qi, h * 64:(h + 1) * 64].double()
                s = [float(qv @ k[r, h, t].double()) / 8 for r, t in zip(row, ts)]
                mx = max(s)
                w = [math.exp(x - mx) for x in s]
                acc = torch.zeros(64, dtype=torch.float64)
                for wi, r, t in zip(w, row, ts):
                    acc += wi * v[r, h, t].double()
                out[b, qi, h * 64:(h + 1) * 64] = acc / sum(w)
    return out


SMALL = ("dec-rmap-shift-step0", "dec-rmap-step1", "dec-seqmap-pad-shift", "pf-nq5-seqmul3", "dec-clamp", "mfma-pad-past-first-queries", "mfma-shift")


@pytest.mark.parametrize("name", SMALL)
def test_reference_is_the_definition(name):
    """Row-map parity, seq_map, seq_mul, pos_shift, the Tmax - 1 clamp and the empty window: the dense f64 reference equals a brute-force loop."""
    c = next(c for c in AM.CASES if c.name == name and c.prec == AM.PREC_F32)
    q, k, v = AM.random_operands(c)
    ref, _ = AM.attend(q, k, v, AM.geometry(c))
    brute = _brute(c, q, k, v)
    assert bool(torch.isfinite(ref).all())
    err = float(((ref - brute).abs() / (1 + brute.abs())).max())
    assert err <= 1e-12, err
    if name == "mfma-pad-past-first-queries":
        assert bool((ref[0, :5] == 0).all()) and bool((ref[0, 5:] != 0).any())
    if name == "dec-clamp":
        assert AM.geometry(c).last.max() == c.Tmax - 1 < c.pos


def test_matrix_names_every_path():
    from indextts_amd import _lib
    assert _lib.attention_path_names() == AM.ALL_PATHS
    L = _lib.lib()
    assert L.itts_attention_path_name(-1) is None and L.itts_attention_path_name(len(AM.ALL_PATHS)) is None
    assert {AM.path_of(c, w) for c in AM.CASES for w in c.waves} == set(AM.ALL_PATHS)
    ids = [AM.case_id(c) for c in AM.CASES]
    assert len(set(ids)) == len(ids)


def test_matrix_holds_the_cases_it_was_built_for():
    has = lambda **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in AM.CASES)
    for prec in (0, 1):
        for nq in (2, 15, 16, 17, 63, 64, 65, 129):
            for pos0 in (0, 1, 63, 64, 65, 200):
                assert has(prec=prec, kind="mfma", nq=nq, pos=pos0)
        assert has(prec=prec, kind="mfma", nq=65, pos=1000) and has(prec=prec, kind="mfma", seq_mul=3) and has(prec=prec, name="mfma-shift")
        pads = {c.pad[b * max(c.seq_mul, 1)] for c in AM.CASES if c.kind == "mfma" and c.prec == prec and c.pad for b in range(3)}
        assert pads >= {0, 1, 15, 16, 17, 63, 64, 65}
        for nq in (2, 5, 65):
            assert has(prec=prec, kind="streams", nq=nq)
        assert has(prec=prec, kind="streams", nq=5, seq_mul=3) and has(prec=prec, kind="streams", nseq=130) and has(prec=prec, Tmax=130, pos=140)
        for rmap in (False, True):
            ns, firsts = set(), set()
            for c in AM.CASES:
                if c.prec == prec and c.name.startswith("keys-") and c.rmap == rmap:
                    g = AM.geometry(c)
                    ns |= set((g.last[:, 0] - g.first + 1).tolist())
                    firsts |= set(g.first.tolist())
                    assert c.waves == (4, 8, 16)
            assert ns == set(AM.KEY_COUNTS) and firsts >= set(AM.FIRSTS)
        for step in (0, 1):
            assert has(prec=prec, rmap=True, step=step, shift=None) and has(prec=prec, name=f"dec-rmap-shift-step{step}")
    assert not any(c.nq > 1 and c.pos + c.nq > c.Tmax for c in AM.CASES)           # no launch the engine never makes
    assert all(c.nq == 1 for c in AM.CASES if c.rmap)


def test_every_table_index_is_in_range():
    for c in AM.CASES:
        g = AM.geometry(c)
        assert 0 <= int(g.pb.min()) and int(g.pb.max()) < AM.ROWS, AM.case_id(c)
        assert 0 <= int(g.rows.min()) and int(g.rows.max()) < AM.ROWS
        for m in AM.row_maps(c.nseq, c.Tmax) if c.rmap else ():
            assert 0 <= int(m.min()) and int(m.max()) < AM.MAP_ROWS
        if c.pad is not None:
            assert len(c.pad) == AM.ROWS and all(0 <= p < c.Tmax for p in c.pad)
        if c.shift is not None:
            assert len(c.shift) == AM.ROWS and all(0 <= s <= c.pos for s in c.shift)
        assert int(g.last.min()) >= 0 and int(g.last.max()) <= c.Tmax - 1
        visible, finite = AM.cells(c)
        assert bool(visible.any()) and not bool(finite[AM.MAP_ROWS:].any() and c.rmap)
    m0, m1 = AM.row_maps(3, 1200)
    assert bool((m0 != m1).all())                                                   # the wrong parity reads another row at every key
    assert all(len(set(m[:, t].tolist())) == 3 for m in (m0, m1) for t in range(0, 1200, 7))


@pytest.mark.parametrize("c", AM.CASES, ids=AM.case_id)
def test_premises_and_mutants(c):
    g = AM.geometry(c)
    n = g.mask.sum(-1)
    # ---- one-hot: the f64 result rounds to the target's V row; the other keys' total weight is below half an ulp of the smallest entry ----
    k0, v, launches = AM.onehot_operands(c)
    vis = torch.isfinite(v) & (v.abs() < 1e29)
    assert float(v[vis].abs().min()) >= 1 and float(v[vis].abs().max()) <= 255 and torch.equal(v[vis], v[vis].round())
    half_ulp = 2.0 ** -9 if c.prec == AM.PREC_BF16 else 2.0 ** -25                 # of the smallest target entry, 1
    assert int(n.max()) * math.exp(-40) * 255 < half_ulp
    for oh in launches:
        k = AM.patched(k0, oh)
        out, _ = AM.attend(oh.q, k, v, g)
        eng = AM.to_engine(out, c.prec)
        assert AM.check_canary(eng) + AM.check_onehot(eng, oh.expect, c.prec) == [], oh.rule
        s = torch.einsum("bqhd,bhtd->bhqt", oh.q.view(c.nseq, c.nq, AM.H, 64).double(),
                         torch.nan_to_num(k[g.rows[:, None, :], torch.arange(AM.H)[None, :, None], torch.arange(c.Tmax)[None, None, :]].double(), nan=0.0)) / 8
        s = torch.where(g.mask[:, None], s, torch.zeros((), dtype=torch.float64))
        assert set(s.unique().tolist()) <= {0.0, 40.0} and bool(((s == 40).sum(-1) == (n > 0)[:, None, :]).all()), oh.rule
    # ---- uniform: exact sums ----
    q, k, v = AM.uniform_operands(c)
    assert float(q.abs().max()) == 0 and int(n.max()) * 255 < 2 ** 24
    # ---- bf16 engine: what the cache holds are bf16 values ----
    qr, kr, vr = AM.random_operands(c)
    if c.prec == AM.PREC_BF16:
        for x in (k0, AM.onehot_operands(c)[1], k, v, kr, vr):
            f = torch.isfinite(x)
            assert torch.equal(x[f].bfloat16().float(), x[f])
    # ---- random: the plain-f32 figure behind the limit is a nonzero finite number ----
    ref, limit, E = AM.random_limit(c, qr, kr, vr)
    assert 0 < E < 1e-4 and math.isfinite(E), E
    assert AM.check_canary(AM.to_engine(ref, c.prec)) + AM.check_random(AM.to_engine(ref, c.prec), ref, limit) == []
    # ---- mutants: every defect that changes what this case reads fails the GPU test's own comparison ----
    for mutant in AM.MUTANTS:
        gm = AM.geometry(c, mutant)
        if gm is None:
            continue
        caught = None
        for L in AM.launches(c):
            if L.label.startswith("onehot") and L.check(AM.to_engine(AM.attend(L.q, L.k, L.v, gm)[0], c.prec)):
                caught = L.label
                break
        assert caught, f"{mutant}: passes every one-hot launch (targets, poison and NaN canaries)"
        BY[mutant, caught.split()[0]] += 1
        if mutant.startswith("drop@") and c.prec == AM.PREC_F32:
            out = AM.to_engine(AM.attend(qr, kr, vr, gm)[0], c.prec)
            assert AM.check_canary(out) + AM.check_random(out, ref, limit), f"{mutant}: inside the random family's limit"


def test_every_mutant_applied_somewhere():
    """After the per-case tests: each deliberate defect changed what at least one case reads (and was caught there); prints, per mutant, the
    one-hot launch that caught it first and in how many cases (run with -s)."""
    for (mutant, fam), n in sorted(BY.items()):
        print(f"{mutant:<18}{fam:<10}{n}")
    if BY:                                                       # (nothing to say when the per-case tests were deselected)
        assert {m for m, _ in BY} == set(AM.MUTANTS)
