"""GPU: every kernel and geometry behind `launch_gemm`, through `itts_gemm_forward`, against an f64 reference at its own tile edges
(tests/gemm_matrix.py: the shapes, the kernel each is meant for, the operands, the bound).  Per case:

  a. the path: the options are set, the GEMM runs, and `itts_gemm_last_path()` must name the kernel the case was built for;
  b. exact-integer operands: the output equals the f64 result BITWISE (any dropped, duplicated or misplaced k-block, row or column shows);
  c. wide-dynamic-range operands: elementwise inside the derived first-order bound of an f32 accumulation;
  canary: the output buffer carries 4096 extra floats behind M * N; they keep their sentinel, and no element of the M * N block keeps the
  NaN it was pre-filled with.

The largest error / bound per path is printed by test_every_reachable_path_was_hit (run with -s); the bound is derived, never fitted to it.
As measured on an MI355X when the matrix was written (every bitwise case equal, every canary intact):

    bf16 tile 128x128 / 256x256 / 256x128   0.012      bf16 slab, 16 / 32 rows             0.004 / 0.007
    bf16 tile 128x128, per-lane epilogue    0.004      bf16 slab, 64 rows, 1 / 2 / 4 nt    0.008 / 0.002 / 0.008
    bf16 register prefill                   0.019      bf16 register decode, mt 1 / 2 / 4  0.007 / 0.007 / 0.007
    f32 tile                                0.055      f32 register decode, mt 1 / 2 / 4   0.085 / 0.081 / 0.073
    f32 register prefill                    0.102      fp32x3 4 waves (6 / 8 products), 8 waves   0.019 / 0.019 / 0.019

(bf16 products are exact in f32, so only the accumulation rounds; the f32 kernels also round every product.)"""
import collections
import ctypes as C

import pytest
import torch

from tests import gemm_matrix as GM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 4096
TAIL_BITS = 0x4B1D4B1D                                                              # behind the output: a finite f32 bit pattern
NAN_BITS = 0x7FC5A5A5                                                               # a quiet NaN with a payload

HIT = collections.defaultdict(int)            # path -> cases that ran on it
RATIO = collections.defaultdict(float)        # path -> largest error / bound


@pytest.fixture(scope="module")
def packed():
    """Packed weights, shared by the cases of one (kind, precision, K, N): packing is host work."""
    cache = {}

    def get(kind, prec, M, N, K):
        from indextts_amd import gpt
        key = (kind, prec, M, N, K)
        if key not in cache:
            a, w, b = GM.int_operands(M, N, K) if kind == "int" else GM.rand_operands(M, N, K, prec == GM.PREC_BF16)
            cache[key] = (gpt.pack_gemm_weight(w, prec).to(DEV), (a.bfloat16() if prec == GM.PREC_BF16 else a).to(DEV).contiguous(), b.to(DEV),
                          GM.ref64(a, w, b), GM.bound(a, w, b, prec))
        return cache[key]
    return get


def _run(c, wp, a, b):
    """One launch into a canary-framed buffer; returns the (M, N) block on the host and the path taken."""
    from indextts_amd import _lib
    L = _lib.lib()
    n = c.M * c.N
    buf = torch.empty(n + PAD, dtype=torch.int32, device=DEV)
    buf[:n] = NAN_BITS
    buf[n:] = TAIL_BITS
    with _lib.option_scope(**dict(c.opts)):
        _lib.check(L.itts_gemm_forward(_lib.ptr(a), _lib.ptr(wp), _lib.ptr(b), C.c_void_p(buf.data_ptr()), c.M, c.N, c.K, c.prec, c.prefill, 0,
                                       _lib.stream_ptr(torch.device(DEV))), "itts_gemm_forward")
        path = _lib.gemm_last_path()
    host = buf.cpu()
    assert bool((host[n:] == TAIL_BITS).all()), f"{int((host[n:] != TAIL_BITS).sum())} floats behind the output were overwritten"
    out = host[:n].view(torch.float32).view(c.M, c.N)
    assert not bool(torch.isnan(out).any()), f"{int(torch.isnan(out).sum())} of {n} output elements were never written"
    return out, path


def _check(c, packed):
    # a + b: the path, exact integers
    wp, a, b, ref, _ = packed("int", c.prec, c.M, c.N, c.K)
    out, path = _run(c, wp, a, b)
    assert path == c.path, f"meant for {c.path}, ran on {path}"
    HIT[path] += 1
    if not torch.equal(out.double(), ref):
        bad = (out.double() != ref).nonzero()
        raise AssertionError(f"{int(bad.shape[0])} of {ref.numel()} elements differ from the f64 result; first at {bad[0].tolist()}: "
                             f"{float(out[tuple(bad[0])])} vs {float(ref[tuple(bad[0])])}; rows {sorted(set(bad[:, 0].tolist()))[:8]} "
                             f"cols {sorted(set(bad[:, 1].tolist()))[:8]}")
    # c: wide dynamic range inside the derived bound
    wp, a, b, ref, bd = packed("rand", c.prec, c.M, c.N, c.K)
    out, path = _run(c, wp, a, b)
    assert path == c.path
    ratio = float(((out.double() - ref).abs() / bd).max())
    RATIO[path] = max(RATIO[path], ratio)
    print(f"{GM.case_id(c)}: largest error / bound = {ratio:.4f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("c", GM.CASES, ids=GM.case_id)
def test_gemm_path_vs_f64(c, packed):
    _check(c, packed)


def test_path_list_is_the_checked_in_one():
    from indextts_amd import _lib
    assert _lib.gemm_path_names() == GM.ALL_PATHS


def test_every_reachable_path_was_hit(packed):
    """Every name of itts_gemm_path_name that itts_gemm_forward can reach ran in this process on a case of the matrix (a path whose cases were
    deselected runs its first case here), and the per-path table of the largest error / bound."""
    from indextts_amd import _lib
    for p in GM.REACHABLE:
        if not HIT[p]:
            _check(next(c for c in GM.CASES if c.path == p), packed)
    names = _lib.gemm_path_names()
    assert [p for p in names if p not in GM.UNREACHABLE and not HIT[p]] == []
    print("path                      cases   largest error / bound")
    for p in names:
        if p not in GM.UNREACHABLE:
            print(f"{p:<26}{HIT[p]:>5}   {RATIO[p]:.4f}")
