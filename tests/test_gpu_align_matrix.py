"""The alignment-export kernel (`attn_align_kernel`, both cache precisions) through its unit entry `itts_gpt_attention_align_forward`, against
an f64 softmax over the cache's own (for bf16: rounded) contents, at the kernel's edges (tests/align_ref.py: the cases, the reference and
the derived bound).  Per case:
  a. the written rows: columns [0, len) within the bound of the reference, exactly 0 where the span runs past the row's last key, finite;
  b. everything else of the output -- columns from len on, rows of other steps / utterances / skipped rows -- keeps its sentinel, and the
     guards around the output and the cache are intact;
  c. cache cells outside every window hold NaN: an out-of-window read shows as a NaN (or a wrong number) in a.
  d. the same launch twice gives the same bits.
The largest error / bound per precision is printed."""
import collections
import ctypes as C

import pytest
import torch

from tests import align_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
RATIO = collections.defaultdict(float)


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).contiguous().to(DEV) if x is not None else None


def _launch(c, q, kbuf, heads=None, n_heads=None):
    from indextts_amd import _lib
    heads = list(c.heads if heads is None else heads)
    K = len(heads)
    n = R.UTTS * R.MAX_NEW * K * c.cap
    out = torch.full((n + 2 * GUARD,), R.SENTINEL, dtype=torch.float32, device=DEV)
    fin = torch.as_tensor(c.finished, dtype=torch.uint8).to(DEV) if c.finished is not None else None
    tabs = [_i32([c.pos]), _i32(c.pad), _i32(c.shift), _i32(c.seq_map), _i32(c.row_slot), _i32([c.step]), _i32(c.row_step0), _i32(c.row_limit)]
    span = _i32(c.spans)
    hl = (C.c_int32 * K)(*heads)
    rc = _lib.lib().itts_gpt_attention_align_forward(
        _lib.ptr(q), C.c_void_p(kbuf.data_ptr() + GUARD * kbuf.element_size()), C.c_void_p(out.data_ptr() + GUARD * 4), _lib.ptr(span), hl,
        K if n_heads is None else n_heads, *[_lib.ptr(t) for t in tabs], _lib.ptr(fin), 3, R.H, c.Tmax, 1, R.MAX_NEW, c.cap, c.prec,
        _lib.stream_ptr(torch.device(DEV)))
    host = out.cpu()
    return rc, host, host[GUARD:-GUARD].view(R.UTTS, R.MAX_NEW, K, c.cap)


def _cache(c, k):
    bf16 = c.prec == R.PREC_BF16
    bits = (k.bfloat16() if bf16 else k).contiguous().flatten()
    buf = torch.full((bits.numel() + 2 * GUARD,), 3.0, dtype=bits.dtype, device=DEV)
    buf[GUARD:-GUARD] = bits.to(DEV)
    return buf


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_alignment_rows_vs_f64(c):
    q, k = R.operands(c)
    kbuf = _cache(c, k)
    qd = q.contiguous().to(DEV)
    rc, raw, out = _launch(c, qd, kbuf)
    assert rc == 0
    assert bool((raw[:GUARD] == R.SENTINEL).all()) and bool((raw[-GUARD:] == R.SENTINEL).all()), "the output's guards were overwritten"
    assert bool((kbuf[:GUARD] == 3.0).all()) and bool((kbuf[-GUARD:] == 3.0).all())
    untouched = torch.ones_like(out, dtype=torch.bool)
    rows = R.reference(c, q, k)
    assert len(rows) == sum(c.expect)
    for u, rstep, ref, lim in rows:
        ln = ref.shape[1]
        got = out[u, rstep, :, :ln].double()
        untouched[u, rstep, :, :ln] = False
        assert bool(torch.isfinite(got).all()), f"utterance {u}: NaN / Inf in the written columns (an out-of-window key was read)"
        err = (got - ref).abs()
        if ln:
            r = float((err / lim).max())
            RATIO[c.prec] = max(RATIO[c.prec], r)
            print(f"{R.case_id(c)} utterance {u} step {rstep}: {ln} columns, largest error {float(err.max()):.3e}, error / bound {r:.4f}")
            assert r <= 1.0, f"utterance {u}: error / bound = {r:.3f}"
            assert bool((got[ref == 0] == 0).all()), "a span key past the row's last key must be exactly 0"
            assert bool((got >= 0).all()) and float(got.sum(1).max()) <= 1 + 1e-6
    assert bool((out[untouched] == R.SENTINEL).all()), \
        f"{int((out[untouched] != R.SENTINEL).sum())} elements outside the written spans were overwritten; first at {(untouched & (out != R.SENTINEL)).nonzero()[0].tolist()}"
    rc2, _, out2 = _launch(c, qd, kbuf)
    assert rc2 == 0 and torch.equal(out.view(torch.int32), out2.view(torch.int32)), "the same launch twice differs bitwise"


def test_a_head_alone_equals_the_head_in_a_pair():
    """two heads in one launch: each one's rows are, bit for bit, those of a launch of that head alone (pair index = position in the list)"""
    c = next(c for c in R.CASES if len(c.heads) == 2 and c.prec == R.PREC_BF16)
    q, k = R.operands(c)
    kbuf, qd = _cache(c, k), q.contiguous().to(DEV)
    _, _, both = _launch(c, qd, kbuf)
    for i, hd in enumerate(c.heads):
        _, _, one = _launch(c, qd, kbuf, heads=[hd])
        assert torch.equal(both[:, :, i].view(torch.int32), one[:, :, 0].view(torch.int32))


def test_entry_refuses_bad_arguments():
    from indextts_amd import _lib
    c = R.CASES[0]
    q, k = R.operands(c)
    kbuf, qd = _cache(c, k), q.contiguous().to(DEV)
    bad = lambda **kw: _launch(c._replace(**{k_: v for k_, v in kw.items() if k_ in c._fields}), qd, kbuf,
                               **{k_: v for k_, v in kw.items() if k_ not in c._fields})
    for kw in (dict(heads=[R.H]), dict(heads=[-1]), dict(heads=[1, 1]), dict(heads=list(range(4)) * 3, n_heads=9), dict(n_heads=0), dict(cap=6),
               dict(cap=1028), dict(cap=0), dict(prec=2), dict(Tmax=12289)):
        rc, raw, _ = bad(**kw)
        assert rc == _lib.ERR_ARG, kw
        assert bool((raw == R.SENTINEL).all()), f"{kw}: a refused launch wrote"
    torch.cuda.synchronize()


def test_zz_report():
    for prec, r in sorted(RATIO.items()):
        print(f"alignment export, {'bf16' if prec else 'f32'} cache: largest error / derived bound over the matrix = {r:.4f}")
