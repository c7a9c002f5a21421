"""The two kernels of the rescoring pass as unit ops.

`itts_gpt_logp_gather_forward` against numpy f64 `log_softmax`.  Gate 2^-21 + 2^-23 |ref|, from the arithmetic: the row maximum is exact, the
exponentials are f32 `expf` values (at most 2 ulp = 2^-22 relative each) summed in f64, so the log of the sum is off by at most 2^-22 absolute;
`x[tok] - max` and the subtraction of the log run in f64; one rounding of the result to f32 adds 2^-24 |ref|.  The gate is 4 x that sum.

`itts_gpt_attention_align_mq_forward` BIT FOR BIT against `itts_gpt_attention_align_forward` called once per query on the same q row, cache
and tables: operands as tests/align_ref.py builds them (scores of standard deviation 2.5, a bf16-representable cache in the bf16 mode, NaN in
every cell outside the windows), its pad / shift / seq_map variants and span kinds."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

from tests import align_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---- logp_gather ---------------------------------------------------------------------------------------------------------------------------
ROLES = ("dominant", "minus_inf", "target_-1", "target_V", "all_minus_inf", "target_on_minus_inf", "plain")


def _logp_case(V, rows, shift, gen):
    ldl = V + 3 + (V % 5)
    x = (torch.randn(rows, ldl, generator=gen, dtype=torch.float32) * 4.0)
    tgt = torch.randint(0, V, (rows,), generator=gen, dtype=torch.int64)
    roles = [ROLES[(r + shift) % len(ROLES)] for r in range(rows)]
    for r, role in enumerate(roles):
        if role == "dominant":                              # one logit 120 above the target's: expf(x[tok] - max) underflows, the answer is finite
            x[r, :V] = torch.rand(V, generator=gen) * 4 - 2
            d = int(tgt[r] + 1) % V if V > 1 else 0
            x[r, d] = 100.0
            x[r, int(tgt[r])] = -20.0
        elif role == "minus_inf":
            m = torch.rand(V, generator=gen) < 0.3
            m[int(tgt[r])] = False
            x[r, :V][m] = -float("inf")
        elif role == "target_-1":
            tgt[r] = -1
        elif role == "target_V":
            tgt[r] = V
        elif role == "all_minus_inf":
            x[r, :V] = -float("inf")
        elif role == "target_on_minus_inf":
            x[r, int(tgt[r])] = -float("inf")
            x[r, (int(tgt[r]) + 1) % V] = 1.0               # (a finite maximum exists, also at V = 5)
        x[r, V:] = torch.tensor([float("nan"), 3e38, float("inf")] * ldl)[: ldl - V]      # garbage past the valid columns
    return x, tgt, ldl, roles


def _logp_reference(x, tgt, V, roles):
    ref = np.zeros(x.shape[0], dtype=np.float64)
    a = x[:, :V].double().numpy()
    for r, role in enumerate(roles):
        if role in ("target_-1", "target_V", "all_minus_inf"):
            continue
        mx = a[r].max()
        ref[r] = (a[r, int(tgt[r])] - mx) - np.log(np.exp(a[r] - mx).sum())
    return ref


@pytest.mark.parametrize("rows", [1, 3, 130])
@pytest.mark.parametrize("V", [5, 257, 8194])
def test_logp_gather_against_f64_log_softmax(V, rows):
    from indextts_amd import _lib
    L = _lib.lib()
    gen = torch.Generator().manual_seed(zlib.crc32(f"logp-{V}-{rows}".encode()))
    worst, seen = 0.0, set()
    for shift in range(len(ROLES)):
        x, tgt, ldl, roles = _logp_case(V, rows, shift, gen)
        seen |= set(roles)
        out = torch.full((rows + 2,), R.SENTINEL, device=DEV)
        xd, td = x.to(DEV), tgt.to(DEV)
        _lib.check(L.itts_gpt_logp_gather_forward(_lib.ptr(xd), _lib.ptr(td), C.c_void_p(out.data_ptr() + 4), rows, V, ldl, _lib.stream_ptr(DEV)),
                   "itts_gpt_logp_gather_forward")
        got = out.cpu().double().numpy()
        assert got[0] == R.SENTINEL and got[-1] == R.SENTINEL, "a write outside out[0 .. rows - 1]"
        got = got[1:-1]
        ref = _logp_reference(x, tgt, V, roles)
        for r, role in enumerate(roles):
            if role in ("target_-1", "target_V", "all_minus_inf"):
                assert got[r] == 0.0 and not np.signbit(got[r]), (role, got[r])
            elif role == "target_on_minus_inf":
                assert got[r] == -np.inf, (role, got[r])
            else:
                assert np.isfinite(got[r]) and np.isfinite(ref[r]), (role, got[r], ref[r])
                gate = 2.0 ** -21 + 2.0 ** -23 * abs(ref[r])
                err = abs(got[r] - ref[r])
                worst = max(worst, err / gate)
                assert err <= gate, (V, rows, r, role, got[r], ref[r], err, gate)
                if role == "dominant":
                    assert ref[r] < -119.0, "the target's exponential must underflow in f32, or the case shows nothing"
    assert seen == set(ROLES)
    print(f"V={V} rows={rows}: worst error / gate = {worst:.3f}")


# ---- attn_align_mq -------------------------------------------------------------------------------------------------------------------------
H, HD, D = R.H, R.HD, R.D
ROW0, TAIL = 2, 3                                            # the launch writes rows ROW0 .. ROW0 + nq - 1 of ROW0 + nq + TAIL


def _mq_case(name, prec, windows, nq, i, cap=16, kinds=None, n_rows=R.ROWS, exact_tmax=None, short=1):
    """len(windows) sequences whose FIRST query sees windows[b] keys (query qi: windows[b] + qi); tables by the bits of i as in
    align_ref._build: 1 seq_map, 2 pos_shift, pads rotated through align_ref.PADS; sequence `short` has q_len = nq - 2 (at least 0)"""
    nseq = len(windows)
    seq_map = tuple((4, 0, 2)[:nseq]) if i & 1 else None
    pbs = list(seq_map) if seq_map else list(range(nseq))
    wl = [w + nq - 1 for w in windows]                      # the LAST query's windows
    firsts = [R.PADS[(i + j) % 4] for j in range(nseq)]
    lasts = [f + n - 1 for f, n in zip(firsts, wl)]
    pos_last = max(lasts)
    shifts = [pos_last - l for l in lasts]
    if not i & 2:                                           # without the table every row ends at the counter: move the pads instead
        firsts = [pos_last - n + 1 for n in wl]
        if min(firsts) < 0:
            pos_last -= min(firsts)
            firsts = [pos_last - n + 1 for n in wl]
        shifts = [0] * nseq
    if exact_tmax:                                          # the cache ends exactly at the last query's key
        firsts = [f + exact_tmax - 1 - pos_last for f in firsts]
        pos_last = exact_tmax - 1
        assert min(firsts) >= 0
    Tmax = exact_tmax or pos_last + 3
    pad = [min(2 + r, Tmax - 1) for r in range(n_rows)]
    shift = [min(1 + r, pos_last) for r in range(n_rows)]
    for pb, f, s in zip(pbs, firsts, shifts):
        pad[pb], shift[pb] = f, s
    kinds = kinds or [R.WRITTEN_KINDS[(i + 2 * j) % len(R.WRITTEN_KINDS)] for j in range(nseq)]
    spans = []
    for k, w in zip(kinds, windows):
        # "early": starts two keys past the FIRST query's window -- all zeros for the early queries, keys for the later ones
        spans.append((w + 1, min(cap, 6)) if k == "early" else R.span_of(k, w + nq - 1, cap))
    q_len = [nq] * nseq
    if nseq > short:
        q_len[short] = max(nq - 2, 0)
    return dict(name=name, prec=prec, nseq=nseq, nq=nq, Tmax=Tmax, pos0=pos_last - (nq - 1), pad=pad, shift=shift if i & 2 else None, seq_map=seq_map,
                pbs=pbs, firsts=firsts, shifts=shifts, spans=spans, heads=R.HEAD_SETS[i % 3], cap=cap, q_len=q_len, n_rows=n_rows)


def _mq_cases():
    out = []
    for prec in (R.PREC_F32, R.PREC_BF16):
        for i, nq in enumerate((1, 3, 9, 17)):              # one tile, a partial tile, 8 + 1, 8 + 8 + 1
            out.append(_mq_case(f"w1-96-800-nq{nq}", prec, (1, 96, 800), nq, i, kinds=("head", "early", "tail")))
        out.append(_mq_case("w5-64-257-nq9-shift-map", prec, (5, 64, 257), 9, 3, kinds=("early", "mid", "past")))
        out.append(_mq_case("w2-1-130-nq17-map", prec, (2, 1, 130), 17, 5, kinds=("full", "early", "mid"), short=0))
        out.append(_mq_case("cap1024-nq9", prec, (810, 1030, 300), 9, 2, cap=1024, kinds=("full", "full", "full")))
        out.append(_mq_case("tile5-nq9", prec, (2900,), 9, 2, kinds=("early",), n_rows=1))       # 15872 / Tmax = 5 queries per block: 5 + 4
        out.append(_mq_case("tile2-nq3", prec, (7000,), 3, 0, kinds=("tail",), n_rows=1))        # 2 queries per block: 2 + 1
        # the largest Tmax the single-query entry accepts: the tile-size clamp reaches 1, the window ends at Tmax - 1
        out.append(_mq_case("tmax12288-nq3", prec, (12288 - 2 - R.PADS[2],), 3, 2, kinds=("past",), n_rows=1, exact_tmax=12288))
    return out


MQ_CASES = _mq_cases()


def _mq_operands(c):
    """q [nseq][nq][D] f32, k [n_rows][H][Tmax][64] f32 holding the cache's values; every cell outside the LAST query's windows is NaN"""
    gen = torch.Generator().manual_seed(zlib.crc32(f"{c['prec']}-{c['name']}".encode()))
    q = torch.randn(c["nseq"], c["nq"], D, generator=gen) * 2.5
    k = torch.randn(c["n_rows"], H, c["Tmax"], HD, generator=gen)
    if c["prec"] == R.PREC_BF16:
        k = k.bfloat16().float()
    seen = torch.zeros(c["n_rows"], c["Tmax"], dtype=torch.bool)
    for pb, f, s in zip(c["pbs"], c["firsts"], c["shifts"]):
        last = min(c["pos0"] + c["nq"] - 1 - s, c["Tmax"] - 1)
        seen[pb, f:last + 1] = True
    return q, torch.where(seen[:, None, :, None], k, torch.full((), float("nan")))


@pytest.mark.parametrize("c", MQ_CASES, ids=lambda c: f"{'bf16' if c['prec'] else 'f32'}-{c['name']}")
def test_align_mq_has_the_bits_of_the_single_query_kernel(c):
    from indextts_amd import _lib
    L = _lib.lib()
    q, k = _mq_operands(c)
    i32 = lambda v: None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)
    qd = q.to(DEV)
    kd = (k.bfloat16() if c["prec"] == R.PREC_BF16 else k).to(DEV).contiguous()
    span, pad, shift, seq_map, q_len = i32(c["spans"]), i32(c["pad"]), i32(c["shift"]), i32(c["seq_map"]), i32(c["q_len"])
    heads = (C.c_int32 * len(c["heads"]))(*c["heads"])
    nseq, nq, cap, K = c["nseq"], c["nq"], c["cap"], len(c["heads"])
    rows = ROW0 + nq + TAIL
    out = torch.full((nseq, rows, K, cap), R.SENTINEL, device=DEV)
    pos = i32([c["pos0"]])
    st = _lib.stream_ptr(DEV)
    _lib.check(L.itts_gpt_attention_align_mq_forward(_lib.ptr(qd), _lib.ptr(kd), _lib.ptr(out), _lib.ptr(span), heads, K, _lib.ptr(pos), _lib.ptr(pad),
                                                     _lib.ptr(shift), _lib.ptr(seq_map), _lib.ptr(q_len), nseq, H, nq, c["Tmax"], 1, ROW0, rows, cap,
                                                     c["prec"], st), "itts_gpt_attention_align_mq_forward")
    got = out.cpu()
    assert not bool(torch.isnan(got).any()), "a key outside the windows was read into the result"
    step = i32([0])
    written = zeros_early = 0
    for qi in range(nq):
        one = torch.full((nseq, 1, K, cap), R.SENTINEL, device=DEV)
        pq = i32([c["pos0"] + qi])
        qq = qd[:, qi].contiguous()
        _lib.check(L.itts_gpt_attention_align_forward(_lib.ptr(qq), _lib.ptr(kd), _lib.ptr(one), _lib.ptr(span), heads, K, _lib.ptr(pq), _lib.ptr(pad),
                                                      _lib.ptr(shift), _lib.ptr(seq_map), None, _lib.ptr(step), None, None, None, nseq, H, c["Tmax"], 1,
                                                      1, cap, c["prec"], st), "itts_gpt_attention_align_forward")
        ref = one.cpu()
        for b in range(nseq):
            if qi < c["q_len"][b]:
                assert torch.equal(got[b, ROW0 + qi].view(torch.int32), ref[b, 0].view(torch.int32)), \
                    f"sequence {b} query {qi}: max |d| = {float((got[b, ROW0 + qi] - ref[b, 0]).abs().max()):.3e}"
                ln = min(c["spans"][b][1], cap)
                assert bool((ref[b, 0, :, ln:] == R.SENTINEL).all()) and (ln == 0 or bool((ref[b, 0, :, :ln] != R.SENTINEL).all()))
                written += 1
                zeros_early += int(bool((ref[b, 0, :, :ln] == 0).all())) if ln else 0
            else:
                assert bool((got[b, ROW0 + qi] == R.SENTINEL).all()), f"sequence {b}: query {qi} >= q_len = {c['q_len'][b]} was written"
    assert bool((got[:, :ROW0] == R.SENTINEL).all()) and bool((got[:, ROW0 + nq:] == R.SENTINEL).all()), "rows outside row0 .. row0 + nq - 1"
    assert written == sum(c["q_len"])
    mass = got[:, ROW0:ROW0 + nq]
    assert float(mass[mass != R.SENTINEL].max()) > 0.0, "no exported weight: the comparison shows nothing"      # (1e-5 per key in a 12 000-key window)
    print(f"{c['name']}: Tmax {c['Tmax']} -> {max(1, min(8, 15872 // c['Tmax']))} queries per block; {written} rows equal, {zeros_early} all-zero rows")


def test_mq_case_list_covers_what_it_claims():
    """host arithmetic only (no launch): tile sizes 1, 2, 5 and 8, full and partial tiles, every table variant, a short q_len, an `early` span"""
    tiles = {max(1, min(8, 15872 // c["Tmax"])) for c in MQ_CASES}
    assert tiles >= {1, 2, 5, 8}
    assert {c["nq"] for c in MQ_CASES} >= {1, 3, 9, 17}
    assert any(c["Tmax"] == 12288 for c in MQ_CASES)
    for name in ("shift", "seq_map"):
        assert {c[name] is None for c in MQ_CASES} == {True, False}, name
    assert any(min(c["q_len"]) < c["nq"] for c in MQ_CASES) and any(min(c["q_len"]) == 0 for c in MQ_CASES)
    for c in MQ_CASES:
        assert all(0 <= f < c["Tmax"] for f in c["firsts"]) and c["pos0"] + c["nq"] - 1 - min(c["shifts"]) <= c["Tmax"] - 1
        for (off, ln), f, s in zip(c["spans"], c["firsts"], c["shifts"]):
            assert off >= 0 and ln >= 0
    # an `early` span lies past the first query's window and inside the last one's
    early = [(c, b) for c in MQ_CASES for b, s in enumerate(c["spans"]) if c["nq"] >= 9 and s[1] == min(c["cap"], 6) and
             s[0] == (c["pos0"] - c["shifts"][b] - c["firsts"][b] + 1) + 1]
    assert early, "no span runs past `last` for the early queries only"
    assert {w for c in MQ_CASES for w in [c["pos0"] - s - f + 1 for s, f in zip(c["shifts"], c["firsts"])]} >= {1, 96, 800}
