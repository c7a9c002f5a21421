"""CPU: the premises of tests/test_gpu_gemm_matrix.py, checked without a device -- the exact-integer operands really are exact (so the GPU
file may ask for bitwise equality with f64), the error bound has room for a correct f32 GEMM, and the matrix names every kernel path."""
import torch

from tests import gemm_matrix as GM


def test_integer_reference_is_a_small_multiple_of_a_quarter():
    """For every shape of the matrix: the f64 result of the integer operands is a multiple of 1/4 below 2^24 -- and so is every partial sum
    (|partial| <= |A| @ |W| + |bias|, the same bound) -- hence exactly representable in f32 whatever the summation order."""
    for prec, M, N, K in GM.SHAPES:
        a, w, b = GM.int_operands(M, N, K)
        ref = GM.ref64(a, w, b)
        assert torch.equal(ref * 4, torch.round(ref * 4)), (M, N, K)
        reach = a.double().abs() @ w.double().abs() + b.double().abs()
        assert float(reach.max()) < 2.0 ** 24, (M, N, K)
        assert torch.equal(ref.float().double(), ref), (M, N, K)
        # the ranges the generator promises
        assert float(a.abs().max()) <= 8 and torch.equal(a, a.round())
        assert float(w.abs().max()) <= 2 and torch.equal(w * 4, (w * 4).round())
        assert float(b.abs().max()) <= 16 and torch.equal(b, b.round())


def test_integer_operands_survive_bf16():
    for prec, M, N, K in GM.SHAPES:
        a, w, b = GM.int_operands(M, N, K)
        assert torch.equal(a.bfloat16().float(), a) and torch.equal(w.bfloat16().float(), w), (M, N, K)


def test_rows_and_columns_differ_in_zero_density():
    """A swapped row of A (column of W) must change the result: neighbouring rows / columns are drawn with different densities of zeros."""
    a, w, _ = GM.int_operands(300, 384, 1280)
    ra, cw = (a == 0).double().mean(1), (w == 0).double().mean(0)
    assert float(ra.max() - ra.min()) > 0.5 and float(cw.max() - cw.min()) > 0.5
    assert not any(torch.equal(a[i], a[i + 1]) for i in range(a.shape[0] - 1))
    assert not any(torch.equal(w[:, j], w[:, j + 1]) for j in range(w.shape[1] - 1))


def test_integer_reference_notices_a_misplaced_block():
    """What the bitwise comparison is for: a dropped or duplicated k-block, two swapped rows of A, two swapped columns of W each change the f64
    result of the integer operands (in nearly every element they touch), whatever the magnitude of the operands."""
    a, w, b = GM.int_operands(65, 264, 256)
    ref = GM.ref64(a, w, b)
    drop = a.clone(); drop[:, 32:64] = 0
    dup = a.clone(); dup[:, 32:64] = a[:, 0:32]
    assert float((GM.ref64(drop, w, b) != ref).double().mean()) > 0.9 and float((GM.ref64(dup, w, b) != ref).double().mean()) > 0.9
    rows = a.clone(); rows[[16, 17]] = a[[17, 16]]
    assert float((GM.ref64(rows, w, b)[16:18] != ref[16:18]).double().mean()) > 0.9
    cols = w.clone(); cols[:, [15, 16]] = w[:, [16, 15]]
    assert float((GM.ref64(a, cols, b)[:, 15:17] != ref[:, 15:17]).double().mean()) > 0.9
    assert float((GM.ref64(a, w, torch.zeros_like(b)) != ref).double().mean()) > 0.9 * float((b != 0).double().mean())


def test_plain_f32_matmul_sits_well_inside_the_bound():
    """The bound is not tight for a correct kernel: torch's own f32 matmul of the random operands stays at or below half of it on every shape."""
    worst = 0.0
    for prec, M, N, K in GM.SHAPES:
        a, w, b = GM.rand_operands(M, N, K, prec == GM.PREC_BF16)
        ref = GM.ref64(a, w, b)
        out = (a @ w + b).double()
        ratio = float(((out - ref).abs() / GM.bound(a, w, b, prec)).max())
        worst = max(worst, ratio)
        assert ratio <= 0.5, (prec, M, N, K, ratio)
    print(f"torch f32 matmul: largest error / bound over {len(GM.SHAPES)} shapes = {worst:.4f}")


def test_bf16_random_operands_hold_bf16_values():
    a, w, _ = GM.rand_operands(129, 132, 128, True)
    assert torch.equal(a.bfloat16().float(), a) and torch.equal(w.bfloat16().float(), w)


def test_matrix_names_every_path():
    """The checked-in list equals the library's (which loads without a device), and the matrix has at least one case for every path that
    itts_gemm_forward can reach."""
    from indextts_amd import _lib
    assert _lib.gemm_path_names() == GM.ALL_PATHS
    assert _lib.lib().itts_gemm_path_name(-1) is None and _lib.lib().itts_gemm_path_name(len(GM.ALL_PATHS)) is None
    assert sorted(GM.REACHABLE + GM.UNREACHABLE) == sorted(GM.ALL_PATHS)
    assert {c.path for c in GM.CASES} == set(GM.REACHABLE)
    ids = [GM.case_id(c) for c in GM.CASES]
    assert len(set(ids)) == len(ids)


def test_matrix_holds_the_shapes_it_was_built_for():
    """The edges the matrix exists for are in it (a refactor of the generator must not drop them silently)."""
    has = lambda **kw: any(all(getattr(c, k) == v for k, v in kw.items()) for c in GM.CASES)
    for M in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129):
        assert has(prec=1, prefill=0, M=M, N=264, K=256)
    for nt in (1, 2, 4):
        assert has(path=f"bf16_slab_mt4_nt{nt}", M=33) and has(path=f"bf16_slab_mt4_nt{nt}", M=129)
    assert has(path="bf16_reg_decode_mt4", K=5120, N=48) and has(path="bf16_reg_decode_mt1", K=96, opts=())
    assert has(path="bf16_tile128", N=132, opts=(("tile256", 1),)) and has(path="bf16_tile128", N=132, opts=(("tile256", 2),))
    for p in ("bf16_tile128", "bf16_tile256", "bf16_tile256x128", "bf16_reg_prefill"):
        assert has(path=p, M=300, N=384) and has(path=p, M=1) and has(path=p, K=64) and has(path=p, K=192)
    assert has(path="bf16_reg_prefill", K=32, opts=(("tile256", 1),)) and has(path="bf16_reg_prefill", K=96, opts=(("tile256", 0),))
    for N, K in ((132, 48), (132, 80), (42, 96)):
        assert has(path="f32_reg_prefill", N=N, K=K, opts=())
    assert max(c.N for c in GM.CASES) <= 520 and sorted({c.K for c in GM.CASES if c.K > 1344}) == [5120]
