"""The GEMM test matrix shared by tests/test_gpu_gemm_matrix.py (GPU) and tests/test_gemm_matrix_host.py (CPU): the tile-edge shapes of every
kernel and geometry behind `launch_gemm`, the kernel each shape is meant for (by the name `itts_gemm_last_path` reports), the two operand
generators and the error bound.

Two kinds of operands per case:

* exact integers -- A integers in [-8, 8], W multiples of 1/4 in [-2, 2], bias integers in [-16, 16]: exact in bf16, in f32 and in the high
  plane of the fp32x3 split, and every partial sum is a multiple of 1/4 below 2^24 (K <= 5120: at most 16 K + 16 = 81 936), so ANY summation
  order in f32 returns exactly the f64 result.  Rows of A and columns of W differ in their density of zeros, so a swapped row / column
  changes the result.
* wide dynamic range (the generator of tests/test_gpu_gemm_x3.py::_errors; A and W rounded to bf16 for precision 1), held elementwise to

      |out - ref64| <= 2 (K + 2) 2^-24 (|A| @ |W| + |bias|)        (+ 4 * 2^-24 |A| @ |W| for fp32x3)

  the first-order worst case of an f32 accumulation in any order with at most 2^-23 relative error per operation (K products, K - 1
  additions inside the sum, the bias addition, two to spare); the fp32x3 term covers the two dropped cross terms (m*l, l*m) of the 6-product
  form.  Derived, not measured.
"""
import collections
import functools

import torch

PREC_F32, PREC_BF16, PREC_X3 = 0, 1, 2

# every name itts_gemm_path_name lists, in its order (compared with the library's list in both test files)
ALL_PATHS = [
    "bf16_tile128", "bf16_tile128_novec", "bf16_tile256", "bf16_tile256x128", "bf16_reg_prefill",
    "bf16_slab_mt1", "bf16_slab_mt2", "bf16_slab_mt4_nt1", "bf16_slab_mt4_nt2", "bf16_slab_mt4_nt4",
    "bf16_reg_decode_mt1", "bf16_reg_decode_mt2", "bf16_reg_decode_mt4",
    "f32_tile", "f32_reg_prefill", "f32_reg_decode_mt1", "f32_reg_decode_mt2", "f32_reg_decode_mt4",
    "x3_4w_p6", "x3_4w_p8", "x3_4w_aplanes", "x3_8w",
    "bf16_ln_decode_4w", "bf16_ln_decode_wide_nt2", "bf16_ln_decode_wide_nt4",
]
# not reachable through itts_gemm_forward: the LayerNorm-fused decode kernels (itts_gemm_ln_forward; held to the two launches they replace by
# tests/test_gpu_gpt.py::test_layernorm_fused_decode_gemm_is_bitwise_the_two_launches, which asserts these names) and the plane-operand form
# of the fp32x3 kernel (s2mel handles only: tests/test_gpu_s2mel_ragged_f64.py)
UNREACHABLE = ["x3_4w_aplanes", "bf16_ln_decode_4w", "bf16_ln_decode_wide_nt2", "bf16_ln_decode_wide_nt4"]
REACHABLE = [p for p in ALL_PATHS if p not in UNREACHABLE]

Case = collections.namedtuple("Case", "prec prefill M N K opts path")


def case_id(c):
    o = ",".join(f"{k}={v}" for k, v in c.opts)
    return f"p{c.prec}-{'pf' if c.prefill else 'dec'}-{c.M}x{c.N}x{c.K}-{o or 'default'}-{c.path}"


def _mt(M):
    return 1 if M <= 16 else 2 if M <= 32 else 4


def _build():
    cases, seen = [], set()

    def add(prec, prefill, M, N, K, path, **opts):
        c = Case(prec, int(prefill), M, N, K, tuple(sorted(opts.items())), path)
        if c[:6] not in seen:
            seen.add(c[:6])
            cases.append(c)

    # ---- bf16 decode, slab kernel (K / 32 even and <= 40 k-blocks): 16 / 32 / 64 rows per block, 1 / 2 / 4 n-tiles per block at 64 rows ----
    def slab(M, N, K, nt=0, **o):
        path = f"bf16_slab_mt{_mt(M)}" if _mt(M) < 4 else f"bf16_slab_mt4_nt{nt or 1}"     # nt = 0: one round of blocks at these sizes -> 1
        add(PREC_BF16, 0, M, N, K, path, decode_gemm=1, decode_nt=nt, **o)

    for M in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129):
        for nt in ((0, 1, 2, 4) if M >= 33 else (0,)):
            slab(M, 264, 256, nt)
    for N in (8, 16, 40, 50, 264, 520):
        for M in (16, 32, 65):
            slab(M, N, 256)
        for nt in (2, 4):                                         # n-tiles past the last one inside a block
            slab(65, N, 256, nt)
    for K in (64, 128, 256, 1280):
        for M in (1, 17, 64):
            slab(M, 264, K)
        slab(64, 264, K, 4)
    for M, N, K in ((65, 264, 1280), (17, 50, 128)):
        slab(M, N, K, decode_rot=0)
        slab(M, N, K, decode_wnt=1)

    # ---- bf16 decode, register path: forced, and where the slab kernel cannot take the K slice ----
    def reg(M, N, K, **o):
        add(PREC_BF16, 0, M, N, K, f"bf16_reg_decode_mt{_mt(M)}", **o)

    for M in (5, 16, 17, 32, 33, 70):
        reg(M, 264, 256, decode_gemm=0)
        for K in (96, 160, 352):                                  # odd k-block counts
            reg(M, 264, K)
    for M in (16, 32, 70):
        for N in (8, 50, 520):
            reg(M, N, 256, decode_gemm=0)
        reg(M, 50, 96)
    for M in (5, 17, 33):
        for K in (64, 1280):
            reg(M, 264, K, decode_gemm=0)
    for M in (5, 17, 70):
        reg(M, 48, 5120)                                          # a slice above 40 k-blocks

    # ---- bf16 prefill: the three tile kernels and the register-path kernel ----
    def pf(M, N, K, variant):
        tiled = K % 64 == 0
        if variant == "reg":
            path, o = "bf16_reg_prefill", {"prefill_gemm": 0}
        else:
            o = {"tile256": variant}
            if not tiled:
                path = "bf16_reg_prefill"
            elif N % 4:
                path = "bf16_tile128_novec"
            elif variant in (1, 2) and N % 128 == 0:
                path = "bf16_tile256" if variant == 1 else "bf16_tile256x128"
            else:
                path = "bf16_tile128"                              # incl. N = 132 under tile256 = 1 / 2, and -1 (pick by shape) at these sizes
        add(PREC_BF16, 1, M, N, K, path, **o)

    for v in (0, 1, 2, "reg"):
        for M in (1, 127, 128, 129, 255, 256, 257, 300):
            pf(M, 256, 128, v)
        for M in (129, 300):                                       # 300 x 384: nine 128-tiles -> 16 blocks, seven idle
            for N in (40, 128, 132, 256, 384):
                pf(M, N, 128, v)
        for K in (64, 128, 192, 1280):
            pf(257, 256, K, v)
        pf(256, 512, 64, v)                                        # exactly 8 tiles of 128 x 128
        pf(300, 512, 64, v)                                        # exactly 8 tiles of 256 x 128
    for v in (-1, 0, 1):
        for K in (32, 96):                                         # K not a multiple of the 64-deep K tile
            pf(129, 256, K, v)
        pf(129, 50, 128, v)                                        # N % 4 != 0: the per-lane epilogue
    pf(129, 50, 128, "reg")
    pf(300, 384, 128, -1)

    # ---- f32: tile kernel, register-path prefill kernel, register-path decode geometries ----
    def f32pf(M, N, K, **o):
        tile_ok = K % 32 == 0 and N % 4 == 0
        path = "f32_tile" if tile_ok and o.get("f32_tile", 1) == 1 else "f32_reg_prefill"
        add(PREC_F32, 1, M, N, K, path, **o)

    for t in (1, 0):
        for M in (1, 127, 128, 129, 255, 256, 257, 300):
            f32pf(M, 256, 96, f32_tile=t)
        for M in (129, 300):
            for N in (40, 128, 132, 256, 384):
                f32pf(M, N, 96, f32_tile=t)
        for K in (16, 32, 96, 512):
            f32pf(257, 132, K, f32_tile=t)
        f32pf(256, 512, 32, f32_tile=t)                            # exactly 8 tiles
    for N, K in ((132, 48), (132, 80), (42, 96)):                  # pf_f32_ok fails: the register path without the option
        f32pf(129, N, K)
    for M in (1, 16, 17, 32, 33, 70):
        add(PREC_F32, 0, M, 264, 96, f"f32_reg_decode_mt{_mt(M)}")
    for M in (16, 32, 70):
        for K in (16, 32, 512):
            add(PREC_F32, 0, M, 264, K, f"f32_reg_decode_mt{_mt(M)}")
        for N in (8, 50, 520):
            add(PREC_F32, 0, M, N, 96, f"f32_reg_decode_mt{_mt(M)}")

    # ---- fp32x3: 4 / 8 waves x 6 / 8 products (the 8-wave kernel exists for 6 products, interleaved split) ----
    def x3(M, N, K, waves, products, **o):
        path = "x3_8w" if (waves, products) == (8, 6) and o.get("x3_sched", 1) == 1 else f"x3_4w_p{products}"
        add(PREC_X3, 1, M, N, K, path, x3_waves=waves, x3_products=products, **o)

    for waves in (4, 8):
        for products in (6, 8):
            for M in (1, 37, 128, 129, 300):
                x3(M, 132, 96, waves, products)
            for M in (129, 300):
                for N in (80, 128, 132, 512):
                    x3(M, N, 96, waves, products)
            for K in (32, 96, 128, 544):
                x3(37, 128, K, waves, products)
    x3(300, 132, 544, 8, 6, x3_sched=0)
    x3(300, 132, 544, 8, 8, x3_sched=0)
    return cases


CASES = _build()
SHAPES = sorted({(c.prec, c.M, c.N, c.K) for c in CASES})


def _seed(M, N, K):
    return M * 1000003 + N * 1009 + K


def _zero_density(n, salt):
    """A different fraction of zeros (5 % .. 85 %) for every row / column: golden-ratio sequence."""
    return 0.05 + 0.8 * ((torch.arange(n, dtype=torch.float64) * 0.6180339887498949 + salt) % 1.0)


@functools.lru_cache(maxsize=None)
def int_operands(M, N, K):
    """(A [M, K], W [K, N], bias [N]) as f32: integers in [-8, 8], multiples of 1/4 in [-2, 2], integers in [-16, 16]."""
    g = torch.Generator().manual_seed(_seed(M, N, K))
    a = torch.randint(-8, 9, (M, K), generator=g).float()
    a = a * (torch.rand(M, K, generator=g, dtype=torch.float64) >= _zero_density(M, 0.1)[:, None]).float()
    w = torch.randint(-8, 9, (K, N), generator=g).float() / 4
    w = w * (torch.rand(K, N, generator=g, dtype=torch.float64) >= _zero_density(N, 0.7)[None, :]).float()
    b = torch.randint(-16, 17, (N,), generator=g).float()
    return a, w, b


@functools.lru_cache(maxsize=None)
def rand_operands(M, N, K, bf16):
    """Wide dynamic range per row of A and per column of W (tests/test_gpu_gemm_x3.py::_errors); bf16: A and W hold bf16 values."""
    g = torch.Generator().manual_seed(_seed(M, N, K) + 1)
    a = torch.randn(M, K, generator=g) * torch.exp(torch.randn(M, 1, generator=g))
    w = torch.randn(K, N, generator=g) * torch.exp(0.5 * torch.randn(1, N, generator=g)) / K ** 0.5
    b = torch.randn(N, generator=g)
    if bf16:
        a, w = a.bfloat16().float(), w.bfloat16().float()
    return a, w, b


def ref64(a, w, b):
    return a.double() @ w.double() + b.double()


def bound(a, w, b, prec):
    K = a.shape[1]
    aw = a.double().abs() @ w.double().abs()
    bd = 2.0 * (K + 2) * 2.0 ** -24 * (aw + b.double().abs())
    if prec == PREC_X3:
        bd = bd + 4.0 * 2.0 ** -24 * aw
    return bd
