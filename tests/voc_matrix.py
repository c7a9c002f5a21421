"""The vocoder test matrix shared by tests/test_gpu_voc_matrix.py (GPU) and tests/test_voc_matrix_host.py (CPU): the tile-edge cases of every
kernel behind the vocoder's conv and activation launchers, the kernel each case is meant for (by the name `itts_voc_last_path` reports), the
operand generators, the f64 references and the bounds.  Style and purpose of tests/gemm_matrix.py.

Convolutions (f32 MFMA conv and its transposed form, bf16 x 3, f16 x 3).  Two kinds of operands per case:

* exact -- x integers in [-8, 8], w multiples of 1/4 in [-2, 2], bias / bias_b / residual / accumulate buffer integers in [-16, 16], div = 4,
  with a density of zeros that differs per input channel, per output channel and per tap.  Every value is exact in bf16 and in f16 (the low
  planes / parts are zero), every partial sum is a multiple of 1/4 with a reach of 16 K + 48 (K = C_in k <= 1056: 16 944, far below 2^24), and
  the division by 4 is exact: ANY f32 evaluation returns exactly the f64 result, in all three modes.  The GPU output is compared BITWISE.
* wide range -- x = N(0,1) times a per-channel log-normal scale, w = N(0,1) times a per-output-channel log-normal scale / sqrt(C_in k),
  the other operands N(0,1), div = 3.  Held by two criteria.

  (a) elementwise, with K = the number of products per output (C_in k; C_in k / u for the transposed conv), XW = |x| (*) |w| and
      S = XW + |bias| + |bias_b| + |res| + |y0|:

          |y - ref64| <= 2 (K + 5) 2^-24 S                                         (/ div under acc_mode 2)

      the first-order worst case of an f32 accumulation in any order (K products, K - 1 additions, at most 2^-23 relative each); the 5
      covers the epilogue: the bias, residual and accumulate additions, the f16 mode's hi + lo addition, the division.  Under acc_mode 2
      everything in front of the division is scaled by 1 / div and the division's own rounding is 2^-24 |ref| <= 2^-24 S / div, so the whole
      bound is divided by div.  bf16 x 3 adds 4 * 2^-24 XW: three dropped plane products (m l, l m, l l) of at most 2^-24 |x w| each, one
      to spare.  f16 x 3 adds 12 * 2^-24 XW + 2^-25 (sum |w| + sum |x| over the window): each operand is carried to 2^-22 relative (two
      terms), the low-by-low product (2^-22) is dropped -- 3 * 2^-22 = 12 * 2^-24 --, and a value below 2^-14 has no high part, only the
      11-bit low part: an absolute error of at most 2^-11 * 2^-14 = 2^-25 per operand, multiplied by the other operand of the product.
      Derived, never fitted.
  (b) (a) is loose at large K (over the matrix a plain f32 evaluation reaches at most 0.14 of it, far less at large K), so a case with at least RMS_MIN_OUTPUTS valid outputs must also
      satisfy rms(y - ref64) <= 1.5 rms(seq32 - ref64), where seq32 is a plain f32 accumulation of the same operands on the CPU, one
      (channel, tap) term at a time, product and sum each rounded, followed by the kernels' epilogue order.  For f16 x 3 the right side is
      1.5 sqrt(rms(seq32 - ref64)^2 + rms(split emulation - ref64)^2); the split emulation applies split_tm_kernel's arithmetic to both
      operands and sums the three products in f64.  The baseline is the reference's own error; the margin 1.5 rests on a CPU check: two
      opposite summation orders of seq32 differ by up to 25 % (log-normal channel scales), a dropped low plane raises the error 4.6 x
      (bf16 x 3) and 360 x (f16 x 3) at C_in 96, k 11; tests/test_voc_matrix_host.py asserts both.

  Ragged batches: row b is min(lens[b] * len_mult, T) frames long; the reference zeroes x beyond that length (the kernels' zero padding at
  the row's own end) and only frames inside the row are compared; frames beyond it must keep the NaN pattern the buffer was filled with.

Anti-aliased activation (aa_v1_sinf, aa_v2_sinf, aa_v2_vsin, aa_planes_vsin).  The reference is the oracle's Activation1d
(oracle/bigvgan_oracle.py::activation1d) evaluated in f64 on the f32 inputs, row by row at the row's own length.  The bound is first order
and propagated stage by stage, with e = 2^-24 and every quantity taken from the f64 reference:

    u  = 2 sum_6 fu x                       E_u   = 6 e (2 |fu| (*) |x|)                              six-term fmaf chain
    a  = exp(alpha), b = exp(beta)          R_a   = 4 e L,  R_b = (4 L + 3) e                         expf: 2 ulp = 4 e (L = logscale); b + 1e-9,
                                                                                                      the division, one to spare
    g  = u a                                E_g   = a E_u + |g| (R_a + e)                             the argument and its product rounding
    s  = sin(g)                             E_s   = E_sin + E_g                                       |cos| <= 1
    v  = u + s^2 / b                        E_v   = E_u + s^2 / b (R_b + 2 e) + 2 |s| / b E_s + e |v| two product roundings, the final add / fma
    y  = sum_12 fd v                        E_y   = |fd| (*) E_v + 12 e (|fd| (*) |v|)                twelve-term fmaf chain

E_sin = 2^-22 for the two libm variants (2 ulp at |s| <= 1) and E_VSIN for aa_v2_vsin / aa_planes_vsin.  The planes kernel is held on its
output: the three planes sum (exactly, to an f32 value) to something inside the same bound, they are bitwise the bf16 three-way split of the
aa_v2_vsin output on the same input, and frames beyond a row's length are zeros in all three planes.

E_VSIN: the absolute error of the default kernels' sine (sin_reduced: two-term Cody-Waite reduction by 2 pi, then the hardware v_sin_f32),
measured through itts_sin_reduced_forward against an f64 sine on 2^20 f32 points across [-pi, pi] plus every f32 within 64 ulp of 0, +-pi/2
and +-pi (tests/test_gpu_voc_matrix.py::test_sin_reduced_probe).  The constant is TWICE the largest measured error: the grid is finite and an
interpolating unit can peak between points.  One condition on it comes from the project, not from the kernel: E_VSIN <= 6e-6, which the 2e-5
unit tolerance at a gain of at most e^0.5 already implies (2 * 1.65 * E <= 2e-5).

Parameter sets of the activation: "mild" (alpha, beta in U(-0.5, 0.5), x ~ 2 N(0,1): the set of the existing tests) and "wide" (log-alpha in
U(-1, 3), log-beta in U(-3, 1), x ~ 30 N(0,1): arguments of thousands of radians, a gain 1 / beta up to 20).  The wide ranges are chosen to
load the argument reduction and the 1 / beta gain; they are NOT read from a checkpoint (there is none in this repository).
"""
import collections
import functools
import math

import torch

from oracle import bigvgan_oracle as O

EPS = 2.0 ** -24
E_SINF = 2.0 ** -22
# the largest |sin_reduced(x) - sin64(x)| on the probe grid, measured on an AMD Instinct MI355X (gfx950), 2026-10-19, and the constant: twice that
E_VSIN_MEASURED = 2.8392117832996455e-07        # at x = 3.1416006088256836, the 1 049 222-point grid of probe_grid()
E_VSIN = 2.0 * E_VSIN_MEASURED
E_VSIN_CAP = 6e-6
RMS_MIN_OUTPUTS = 4096
RMS_MARGIN = 1.5

# every name itts_voc_path_name lists, in its order (compared with the library's list in both test files)
ALL_PATHS = [
    "conv_f32_bm32", "conv_f32_bm64", "conv_f32_bm96", "conv_f32_bm128",
    "conv_x3_nh1", "conv_x3_nh2",
    "conv_h3_two_stage", "conv_h3_win256x128", "conv_h3_win192x192", "conv_h3_win256x96",
    "aa_v1_sinf", "aa_v2_sinf", "aa_v2_vsin", "aa_planes_vsin",
]
CONV_PATHS = [p for p in ALL_PATHS if p.startswith("conv_")]
ACT_PATHS = [p for p in ALL_PATHS if p.startswith("aa_")]

# ---- tile constants of the kernels (bigvgan_kernels.hip, bigvgan_x3.hip, bigvgan_h3.hip) ----
CONV_HALO = 64
F32_FRAME_TILE = {32: 256, 64: 256, 96: 256, 128: 128}
F32_T = (1, 31, 255, 256, 257, 513)
F32_T_BM128 = (127, 128, 129)
F32_COUT = {32: (1, 24, 31, 32, 33, 48), 64: (63, 64, 65), 96: (95, 96, 97, 200), 128: (127, 128, 129, 200)}
F32_CIN = (8, 24, 32, 40, 80)
F32_KD = ((1, 1), (3, 1), (7, 3), (11, 5), (3, 32))
XCD_TILES = (1, 7, 8, 9, 17)
CONVT_KU = ((8, 4), (4, 2), (12, 4), (2, 2), (4, 4))
CONVT_TIN = (1, 2, 255, 256, 257)
X3_T = (1, 15, 16, 17, 255, 256, 257, 513)
X3_COUT = (1, 48, 96, 97, 192, 193, 384)
X3_CIN = (32, 64, 96)
X3_KD = ((3, 1), (7, 3), (11, 5), (5, 16), (3, 32))
H3_TWO_T = (1, 127, 128, 129)
H3_TWO_COUT = (1, 127, 128, 129, 200)
H3_WIN = {"conv_h3_win256x128": ((97, 128, 200), (255, 256, 257)), "conv_h3_win192x192": ((130, 191, 192), (191, 192, 193)),
          "conv_h3_win256x96": ((80, 96, 270, 288), (255, 256, 257))}
H3_WIN_KD = ((3, 1), (7, 3), (11, 4), (5, 12))            # (k - 1) d <= 48: the last one exactly
ACT_T = (1, 2, 5, 6, 7, 12, 13, 127, 128, 129, 1023, 1024, 1025, 1026, 2049)
ACT_C = {"aa_v1_sinf": (1, 3), "aa_v2_sinf": (1, 3), "aa_v2_vsin": (1, 3), "aa_planes_vsin": (8, 24, 32, 40)}
ACT_OPT = {"aa_v1_sinf": 0, "aa_v2_sinf": 1, "aa_v2_vsin": 2, "aa_planes_vsin": 2}
ACT_TILE = {"aa_v1_sinf": 1024, "aa_v2_sinf": 1024, "aa_v2_vsin": 1024, "aa_planes_vsin": 128}

# op: "f32" / "x3" / "h3" (Conv1d, d = dilation) or "convT" (ConvTranspose1d, d = stride u, T = input frames)
# epi: none | bias | biasb | res | acc1 | acc2 | full (everything the mode has, acc_mode 2)
Conv = collections.namedtuple("Conv", "op B Cin Cout T k d lens lm epi opts path")
Act = collections.namedtuple("Act", "B C T lens lm logscale pset opts path")
EPILOGUES = {"f32": ("none", "bias", "biasb", "res", "acc1", "acc2"), "x3": ("none", "bias", "res", "acc1", "acc2"),
             "h3": ("none", "bias", "res", "acc1", "acc2"), "convT": ("none", "bias", "biasb")}


def conv_id(c):
    o = ",".join(f"{k}={v}" for k, v in c.opts) or "default"
    ln = "full" if c.lens is None else "l" + "_".join(map(str, c.lens)) + f"x{c.lm}"
    return f"{c.op}-B{c.B}-{c.Cin}to{c.Cout}-T{c.T}-k{c.k}d{c.d}-{ln}-{c.epi}-{o}-{c.path}"


def act_id(c):
    ln = "full" if c.lens is None else "l" + "_".join(map(str, c.lens)) + f"x{c.lm}"
    return f"{c.path}-B{c.B}-C{c.C}-T{c.T}-{ln}-log{c.logscale}-{c.pset}"


def h3_path(Cout, k, d, h3_kernel=1):
    """The dispatch of launch_conv_h3: the window kernel where the taps fit, with the co tile that pads the fewest columns."""
    if not (h3_kernel != 0 and k >= 3 and (k - 1) * d <= 48):
        return "conv_h3_two_stage"
    padded = lambda bn: -(-Cout // bn) * bn
    best = 128
    if padded(192) < padded(best):
        best = 192
    if padded(96) < padded(best):
        best = 96
    return {128: "conv_h3_win256x128", 192: "conv_h3_win192x192", 96: "conv_h3_win256x96"}[best]


def _cyc(A, B, n=1):
    """Pairs that cover every value of A and of B (n + 1 partners each way), not their full product."""
    out = []
    for i in range(max(len(A), len(B))):
        for s in range(n + 1):
            p = (A[i % len(A)], B[(i + s) % len(B)])
            if p not in out:
                out.append(p)
    return out


def ragged(T):
    """lens with 0, 1, T and a value above T"""
    return (0, 1, T, T + 5)


def ragged2(T):
    """len_mult = 2 with halved lens: rows of 0, 2, 2 (T // 2) and T frames"""
    return (0, 1, T // 2, T)


def _build_conv():
    cases, seen = [], set()

    def add(op, B, Cin, Cout, T, k, d, path, lens=None, lm=1, epi="bias", **opts):
        if lens is not None:
            B = len(lens)
        c = Conv(op, B, Cin, Cout, T, k, d, lens, lm, epi, tuple(sorted(opts.items())), path)
        if c not in seen:
            seen.add(c)
            cases.append(c)

    # ---- f32 MFMA conv: four co-tile heights (option conv_bm; 0 = 32) ----
    for bm in (32, 64, 96, 128):
        path, ft = f"conv_f32_bm{bm}", F32_FRAME_TILE[bm]
        o = {} if bm == 32 else {"conv_bm": bm}
        Ts = F32_T_BM128 if bm == 128 else F32_T
        for T, Cout in _cyc(Ts, F32_COUT[bm], 1 if bm == 32 else 0):
            add("f32", 2, 24, Cout, T, 7, 3, path, **o)
        for Cin, (k, d) in (((a, b) for a in F32_CIN for b in F32_KD) if bm == 32 else _cyc(F32_CIN, F32_KD, 0)):
            add("f32", 1, Cin, bm + 1, ft + 1, k, d, path, **o)
        T = ft + 1
        for epi in EPILOGUES["f32"]:
            add("f32", 2, 40, bm + 8, T, 3, 1, path, epi=epi, **o)
        for epi in (EPILOGUES["f32"] if bm == 32 else ("full",)):
            add("f32", 0, 40, bm + 8, T, 7, 3, path, lens=ragged(T), epi=epi, **o)
            add("f32", 0, 40, bm + 8, T, 7, 3, path, lens=ragged2(T), lm=2, epi=epi, **o)
        for tiles in XCD_TILES:                                    # B * n_frame_tiles, with one and with three channel tiles
            for nco in (1, 3):
                B, nt = {1: (1, 1), 7: (7, 1), 8: (4, 2), 9: (3, 3), 17: (17, 1)}[tiles]
                add("f32", B, 8, bm * nco - 1, ft * nt - 3, 3, 1, path, conv_bm=bm)
    # ---- transposed conv: u phase launches on the f32 kernel, at conv_bm 0 and 128 ----
    for bm in (0, 128):
        path = "conv_f32_bm128" if bm else "conv_f32_bm32"
        for (k, u), Tin in _cyc(CONVT_KU, CONVT_TIN, 2):
            add("convT", 2, 24, 40, Tin, k, u, path, conv_bm=bm)
        for epi in EPILOGUES["convT"]:
            add("convT", 2, 40, 33, 129, 8, 4, path, epi=epi, conv_bm=bm)
            add("convT", 0, 40, 33, 129, 12, 4, path, lens=ragged(129), epi=epi, conv_bm=bm)
        add("convT", 0, 40, 33, 130, 4, 2, path, lens=ragged2(130), lm=2, epi="biasb", conv_bm=bm)
    # ---- bf16 x 3 window kernel: one / two co tiles of 96 per window ----
    x3p = lambda Cout: "conv_x3_nh2" if Cout > 96 else "conv_x3_nh1"
    for T, Cout in _cyc(X3_T, X3_COUT, 1):
        add("x3", 2, 32, Cout, T, 7, 3, x3p(Cout))
    for Cin, (k, d) in ((a, b) for a in X3_CIN for b in X3_KD):
        for Cout in (97, 48):
            add("x3", 1, Cin, Cout, 257, k, d, x3p(Cout))
    for Cout in (96, 193):
        for epi in EPILOGUES["x3"]:
            add("x3", 2, 32, Cout, 257, 3, 1, x3p(Cout), epi=epi)
        for epi in ("bias", "full"):
            add("x3", 0, 32, Cout, 260, 7, 3, x3p(Cout), lens=ragged(260), epi=epi)
            add("x3", 0, 32, Cout, 260, 7, 3, x3p(Cout), lens=ragged2(260), lm=2, epi=epi)
        for tiles in XCD_TILES:
            add("x3", tiles, 32, Cout, 250, 3, 1, x3p(Cout))
    # ---- f16 x 3: the two-stage kernel (k = 1, (k - 1) d > 48, or option h3_kernel = 0) and the three window tiles ----
    for T, Cout in _cyc(H3_TWO_T, H3_TWO_COUT, 1):
        add("h3", 2, 32, Cout, T, 7, 3, "conv_h3_two_stage", h3_kernel=0)
    for k, d in ((1, 1), (11, 5), (3, 32), (3, 25)):
        for Cin in (32, 96):
            assert h3_path(129, k, d) == "conv_h3_two_stage"
            add("h3", 1, Cin, 129, 129, k, d, "conv_h3_two_stage")
    for epi in EPILOGUES["h3"]:
        add("h3", 2, 64, 129, 129, 3, 1, "conv_h3_two_stage", epi=epi, h3_kernel=0)
    for epi in ("bias", "full"):
        add("h3", 0, 32, 129, 132, 11, 5, "conv_h3_two_stage", lens=ragged(132), epi=epi)
        add("h3", 0, 32, 129, 132, 11, 5, "conv_h3_two_stage", lens=ragged2(132), lm=2, epi=epi)
    for path, (Couts, Ts) in H3_WIN.items():
        for T, Cout in _cyc(Ts + (1, 513), Couts, 1):
            assert h3_path(Cout, 7, 3) == path
            add("h3", 2, 32, Cout, T, 7, 3, path)
        for Cin, (k, d) in _cyc(X3_CIN, H3_WIN_KD, 1):
            add("h3", 1, Cin, Couts[0], Ts[2], k, d, path)
        for epi in EPILOGUES["h3"]:
            add("h3", 2, 32, Couts[-1], Ts[2], 3, 1, path, epi=epi)
        T = Ts[2] + 3
        for epi in ("bias", "full"):
            add("h3", 0, 32, Couts[-1], T, 7, 3, path, lens=ragged(T), epi=epi)
            add("h3", 0, 32, Couts[-1], T, 7, 3, path, lens=ragged2(T), lm=2, epi=epi)
        for tiles in (7, 9):
            add("h3", tiles, 32, Couts[-1], 190, 3, 1, path)
    return cases


def _build_act():
    cases = []
    for path in ACT_PATHS:
        o, tile = (("aa_act", ACT_OPT[path]),), ACT_TILE[path]
        for i, T in enumerate(ACT_T):
            for p, pset in enumerate(("mild", "wide")):
                C = ACT_C[path][(i + p) % len(ACT_C[path])]
                lens, lm = None, 1
                if T >= 127 and (i + p) % 3 == 0:                  # 0, 1, a tile edge +- 1, a value above T
                    e = tile if tile + 1 <= T else 128 if 129 <= T else T - 1
                    lens = (0, 1, e - 1, e + 1, T + 3)
                elif T >= 12 and (i + p) % 3 == 1:
                    lens, lm = ragged2(T), 2
                cases.append(Act(len(lens) if lens else 2, C, T, lens, lm, (i // 2 + p) % 2, pset, o, path))
    return cases


CONV_CASES = _build_conv()
ACT_CASES = _build_act()


# ---------------------------------------------------------------------------------------------------------------
# convolution operands, references, bounds
# ---------------------------------------------------------------------------------------------------------------
def _seed(c):
    return (c.Cin * 1000003 + c.Cout * 10007 + c.T * 101 + c.k * 13 + c.d + c.B * 7919 + {"f32": 0, "x3": 1, "h3": 2, "convT": 3}[c.op]) % (2 ** 31)


def _dens(n, salt):
    """A different fraction of zeros (5 % .. 65 %) per index: golden-ratio sequence."""
    return 0.05 + 0.6 * ((torch.arange(n, dtype=torch.float64) * 0.6180339887498949 + salt) % 1.0)


def w_shape(c):
    return (c.Cin, c.Cout, c.k) if c.op == "convT" else (c.Cout, c.Cin, c.k)


def t_out(c):
    return c.T * c.d if c.op == "convT" else c.T


def n_terms(c):
    return c.Cin * (c.k // c.d) if c.op == "convT" else c.Cin * c.k


def flags(c):
    """(bias, bias_b, res, acc_mode) of the case's epilogue"""
    e = c.epi
    if e == "full":
        return True, c.op in ("f32", "convT"), c.op != "convT", 0 if c.op == "convT" else 2
    return e == "bias", e == "biasb", e == "res", {"acc1": 1, "acc2": 2}.get(e, 0)


Operands = collections.namedtuple("Operands", "x w bias bias_b res y0 div")


def weight_key(c):
    """What a case's weights depend on -- and with them the packed form, which the GPU test caches: (kind of packing, C_in, C_out, k, stride)"""
    return ("convT" if c.op == "convT" else "conv", c.Cin, c.Cout, c.k, c.d if c.op == "convT" else 0)


@functools.lru_cache(maxsize=None)
def weights(wkey, kind):
    """Conv1d [Cout][Cin][k] / ConvTranspose1d [Cin][Cout][k] weights of one (C_in, C_out, k): shared by every mode, T, batch and epilogue"""
    op, Cin, Cout, k, u = wkey
    g = torch.Generator().manual_seed((Cin * 1000003 + Cout * 10007 + k * 13 + u) * 2 + (0 if kind == "exact" else 1))
    ws = (Cin, Cout, k) if op == "convT" else (Cout, Cin, k)
    co_ax, ci_ax = (1, 0) if op == "convT" else (0, 1)
    shp = lambda ax, n: [n if i == ax else 1 for i in range(3)]
    if kind == "exact":
        w = torch.randint(-8, 9, ws, generator=g).float() / 4
        dens = (_dens(Cout, 0.7).view(shp(co_ax, Cout)) + _dens(Cin, 0.3).view(shp(ci_ax, Cin)) + _dens(k, 0.5).view(shp(2, k))) / 3
        return w * (torch.rand(ws, generator=g, dtype=torch.float64) >= dens).float()
    sc = torch.exp(0.5 * torch.randn(Cout, generator=g)).view(shp(co_ax, Cout))
    return torch.randn(ws, generator=g) * sc / (Cin * k) ** 0.5


@functools.lru_cache(maxsize=8)
def _operands(key, kind):
    c = Conv(*key)
    g = torch.Generator().manual_seed(_seed(c) + (0 if kind == "exact" else 1))
    To = t_out(c)
    w = weights(weight_key(c), kind)
    if kind == "exact":
        x = torch.randint(-8, 9, (c.B, c.Cin, c.T), generator=g).float()
        x = x * (torch.rand(c.B, c.Cin, c.T, generator=g, dtype=torch.float64) >= _dens(c.Cin, 0.1)[None, :, None]).float()
        ri = lambda *s: torch.randint(-16, 17, s, generator=g).float()
        return Operands(x, w, ri(c.Cout), ri(c.B, c.Cout), ri(c.B, c.Cout, To), ri(c.B, c.Cout, To), 4.0)
    x = torch.randn(c.B, c.Cin, c.T, generator=g) * torch.exp(torch.randn(1, c.Cin, 1, generator=g))
    rn = lambda *s: torch.randn(s, generator=g)
    return Operands(x, w, rn(c.Cout), rn(c.B, c.Cout), rn(c.B, c.Cout, To), rn(c.B, c.Cout, To), 3.0)


def _shape_key(c):
    """The fields the operands depend on (lens / epilogue / options select among them, the path is a consequence)."""
    return (c.op, c.B, c.Cin, c.Cout, c.T, c.k, c.d, None, 1, "", (), "")


def operands(c, kind):
    return _operands(_shape_key(c), kind)


def row_lens(c):
    """(input frames, output frames) of every row"""
    To = t_out(c)
    if c.lens is None:
        return [c.T] * c.B, [To] * c.B
    up = c.d if c.op == "convT" else 1
    return [min(n * c.lm, c.T) for n in c.lens], [min(n * c.lm * up, To) for n in c.lens]


def valid_mask(c):
    _, lo = row_lens(c)
    t = torch.arange(t_out(c))
    return (t[None, :] < torch.tensor(lo)[:, None])[:, None, :].expand(c.B, c.Cout, t_out(c))


def zero_beyond(c, x):
    li, _ = row_lens(c)
    t = torch.arange(c.T)
    return x * (t[None, :] < torch.tensor(li)[:, None])[:, None, :].to(x.dtype)


def _shift(x, off):
    """x[..., t + off], zero outside"""
    T = x.shape[-1]
    y = torch.zeros_like(x)
    lo, hi = max(0, -off), min(T, T - off)
    if lo < hi:
        y[..., lo:hi] = x[..., lo + off:hi + off]
    return y


def conv_lin(c, x, w, drop_tap=None, shift_tap=None):
    """The linear part in the dtype of x / w (f64 for the reference): [B][Cout][T_out].  x is already zeroed beyond each row's length.
    drop_tap / shift_tap: the defects of tests/test_voc_matrix_host.py (a tap left out; a tap read one frame off)."""
    if c.op == "convT":
        u, p = c.d, (c.k - c.d) // 2
        full = torch.zeros(c.B, c.Cout, c.T * u + c.k + 1, dtype=x.dtype)
        for j in range(c.k):
            if j == drop_tap:
                continue
            s = j + (1 if j == shift_tap else 0)
            full[:, :, s:s + c.T * u:u] += torch.einsum("co,bct->bot", w[:, :, j], x)
        return full[:, :, p:p + c.T * u].contiguous()
    pad = (c.k - 1) // 2 * c.d
    y = torch.zeros(c.B, c.Cout, c.T, dtype=x.dtype)
    for j in range(c.k):
        if j == drop_tap:
            continue
        y += torch.einsum("oc,bct->bot", w[:, :, j], _shift(x, j * c.d - pad + (1 if j == shift_tap else 0)))
    return y


def epilogue(c, lin, ops, dt):
    """The kernels' epilogue order in dtype dt: (lin + (bias + bias_b)) + res, then y0 + v, then / div"""
    hb, hbb, hr, acc = flags(c)
    v = lin
    if hb or hbb:
        add = torch.zeros(c.B, c.Cout, dtype=dt)
        if hb:
            add = add + ops.bias.to(dt)[None, :]
        if hbb:
            add = add + ops.bias_b.to(dt)
        v = v + add[:, :, None]
    if hr:
        v = v + ops.res.to(dt)
    if acc:
        v = ops.y0.to(dt) + v
        if acc == 2:
            v = v / torch.tensor(ops.div, dtype=dt)
    return v


def ref64(c, ops, **defect):
    return epilogue(c, conv_lin(c, zero_beyond(c, ops.x.double()), ops.w.double(), **defect), ops, torch.float64)


def seq32(c, ops, reverse=False):
    """Plain f32 accumulation, one (channel, tap) term at a time, product and sum each rounded; then the epilogue in f32."""
    x, w = zero_beyond(c, ops.x), ops.w
    To = t_out(c)
    u, p = (c.d, (c.k - c.d) // 2) if c.op == "convT" else (1, 0)
    pad = (c.k - 1) // 2 * c.d
    acc = torch.zeros(c.B, c.Cout, To + (c.k + 1 if c.op == "convT" else 0))
    order = [(ci, j) for ci in range(c.Cin) for j in range(c.k)]
    for ci, j in (reversed(order) if reverse else order):
        if c.op == "convT":
            acc[:, :, j:j + c.T * u:u] += w[ci, :, j][None, :, None] * x[:, ci, None, :]
        else:
            off = j * c.d - pad
            lo, hi = max(0, -off), min(c.T, c.T - off)
            if lo < hi:
                acc[:, :, lo:hi] += w[:, ci, j][None, :, None] * x[:, ci, None, lo + off:hi + off]
    if c.op == "convT":
        acc = acc[:, :, p:p + To].contiguous()
    return epilogue(c, acc, ops, torch.float32)


def split_h3(f):
    """split_tm_kernel's / conv_h3_pack's arithmetic: hi = f16(f) (0 below 2^-14), lo = f16(2^11 (f - hi)); returns (hi, lo) as f64"""
    h = torch.where(f.abs() < 6.103515625e-05, torch.zeros_like(f), f.half().float())
    l = ((f - h) * 2048.0).half().float()
    return h.double(), l.double()


def split_x3(f):
    """split_tm3_kernel's / conv_x3_pack's arithmetic: three bf16 planes, h + m + l == f"""
    h = f.bfloat16().float()
    r = f - h
    m = r.bfloat16().float()
    l = (r - m).bfloat16().float()
    return h, m, l


def split_emulation(c, ops):
    """The products the split-operand kernels keep, summed in f64, with the f64 epilogue."""
    x, w = zero_beyond(c, ops.x), ops.w
    if c.op == "h3":
        xh, xl = split_h3(x)
        wh, wl = split_h3(w)
        lin = conv_lin(c, xh, wh + wl / 2048.0) + conv_lin(c, xl, wh) / 2048.0
    else:
        (xh, xm, xl), (wh, wm, wl) = split_x3(x), split_x3(w)
        d = lambda t: t.double()
        lin = conv_lin(c, d(xh), d(w)) + conv_lin(c, d(xm), d(wh) + d(wm)) + conv_lin(c, d(xl), d(wh))
    return epilogue(c, lin, ops, torch.float64)


def xw_abs(c, ops):
    return conv_lin(c, zero_beyond(c, ops.x.double().abs()), ops.w.double().abs())


def split_term(c, ops, xw=None):
    """What criterion (a) adds for the split-operand modes (0 for the f32 kernel)."""
    if c.op not in ("x3", "h3"):
        return 0.0
    xw = xw_abs(c, ops) if xw is None else xw
    if c.op == "x3":
        return 4.0 * EPS * xw
    x = zero_beyond(c, ops.x.double().abs())
    ones_x = zero_beyond(c, torch.ones_like(x))
    window = conv_lin(c, ones_x, ops.w.double().abs()) + conv_lin(c, x, torch.ones_like(ops.w.double()))
    return 12.0 * EPS * xw + 2.0 ** -25 * window


def bound(c, ops):
    hb, hbb, hr, acc = flags(c)
    xw = xw_abs(c, ops)
    S = xw.clone()
    if hb:
        S += ops.bias.double().abs()[None, :, None]
    if hbb:
        S += ops.bias_b.double().abs()[:, :, None]
    if hr:
        S += ops.res.double().abs()
    if acc:
        S += ops.y0.double().abs()
    bd = 2.0 * (n_terms(c) + 5) * EPS * S + split_term(c, ops, xw)
    return bd / ops.div if acc == 2 else bd


def rms(d, mask):
    d = d.double()[mask]
    return float(d.pow(2).mean().sqrt()) if d.numel() else 0.0


def carries_rms(c):
    return int(valid_mask(c).sum()) >= RMS_MIN_OUTPUTS


def rms_limit(c, ops, ref=None):
    """The right side of criterion (b)."""
    ref = ref64(c, ops) if ref is None else ref
    m = valid_mask(c)
    base = rms(seq32(c, ops).double() - ref, m) ** 2
    if c.op == "h3":
        base += rms(split_emulation(c, ops) - ref, m) ** 2
    return RMS_MARGIN * math.sqrt(base)


# ---------------------------------------------------------------------------------------------------------------
# activation operands, reference, bound
# ---------------------------------------------------------------------------------------------------------------
ActOperands = collections.namedtuple("ActOperands", "x alpha beta")          # alpha, beta as handed to the kernel (log scale iff c.logscale)


@functools.lru_cache(maxsize=None)
def act_operands(c):
    g = torch.Generator().manual_seed(c.C * 100003 + c.T * 31 + c.B * 7 + (1 if c.pset == "wide" else 0) + 2 * c.logscale)
    if c.pset == "mild":
        la, lb = torch.rand(c.C, generator=g) - 0.5, torch.rand(c.C, generator=g) - 0.5
        x = 2.0 * torch.randn(c.B, c.C, c.T, generator=g)
    else:
        la, lb = torch.rand(c.C, generator=g) * 4 - 1, torch.rand(c.C, generator=g) * 4 - 3
        x = 30.0 * torch.randn(c.B, c.C, c.T, generator=g)
    if not c.logscale:
        la, lb = la.double().exp().float(), lb.double().exp().float()
    return ActOperands(x, la, lb)


def act_row_lens(c):
    return [c.T] * c.B if c.lens is None else [min(n * c.lm, c.T) for n in c.lens]


def act_valid(c):
    t = torch.arange(c.T)
    return (t[None, :] < torch.tensor(act_row_lens(c))[:, None])[:, None, :].expand(c.B, c.C, c.T)


def e_sin(path):
    return E_VSIN if path.endswith("vsin") else E_SINF


def _act_row(x, al, be, logscale, esin, fu, fd):
    """(ref, bound) of one row [1][C][n] in f64: the stages of the module docstring."""
    x = x.double()
    fu, fd = fu.double(), fd.double()
    L = 1.0 if logscale else 0.0
    a = (al.double().exp() if logscale else al.double()).view(1, -1, 1)
    b = (be.double().exp() if logscale else be.double()).view(1, -1, 1)
    u = O.upsample2x(x, fu)
    E_u = 6.0 * EPS * O.upsample2x(x.abs(), fu.abs())
    R_a, R_b = 4.0 * EPS * L, (4.0 * L + 3.0) * EPS
    g = u * a
    E_g = a * E_u + g.abs() * (R_a + EPS)
    s = torch.sin(g)
    E_s = esin + E_g
    ib = 1.0 / (b + O.NO_DIV_BY_ZERO)
    v = u + ib * s * s
    E_v = E_u + ib * s * s * (R_b + 2.0 * EPS) + 2.0 * s.abs() * ib * E_s + EPS * v.abs()
    y = O.downsample2x(v, fd)
    E_y = O.downsample2x(E_v, fd.abs()) + 12.0 * EPS * O.downsample2x(v.abs(), fd.abs())
    return y, E_y


def act_ref_bound(c, ops=None, esin=None):
    """(ref [B][C][T] f64, bound, valid mask): every row at its own length through the oracle's stages; 0 beyond the row."""
    ops = act_operands(c) if ops is None else ops
    esin = e_sin(c.path) if esin is None else esin
    f = O.default_filter()
    ref = torch.zeros(c.B, c.C, c.T, dtype=torch.float64)
    bd = torch.zeros_like(ref)
    for b, n in enumerate(act_row_lens(c)):
        if n > 0:
            ref[b:b + 1, :, :n], bd[b:b + 1, :, :n] = _act_row(ops.x[b:b + 1, :, :n], ops.alpha, ops.beta, c.logscale, esin, f, f)
    return ref, bd, act_valid(c)


def act_f32(c, ops=None):
    """torch's f32 evaluation of the same definition (the oracle as the existing tests run it), row by row"""
    ops = act_operands(c) if ops is None else ops
    y = torch.zeros(c.B, c.C, c.T)
    for b, n in enumerate(act_row_lens(c)):
        if n > 0:
            y[b:b + 1, :, :n] = O.activation1d(ops.x[b:b + 1, :, :n], ops.alpha, ops.beta, logscale=bool(c.logscale))
    return y


# ---------------------------------------------------------------------------------------------------------------
# the sine probe
# ---------------------------------------------------------------------------------------------------------------
def _neighbours(vals, n):
    """every f32 within n ulp of the f32 values `vals` (bit patterns +- n; around 0 on both signs)"""
    out = []
    for v in vals:
        bits = torch.tensor([v], dtype=torch.float32).view(torch.int32)
        if v == 0.0:
            mag = torch.arange(0, n + 1, dtype=torch.int32)
            out += [mag.view(torch.float32), (mag | torch.tensor(-2 ** 31, dtype=torch.int32)).view(torch.float32)]
        else:
            out.append((bits + torch.arange(-n, n + 1, dtype=torch.int32)).view(torch.float32))
    return torch.cat(out)


def probe_grid():
    """2^20 f32 points across [-pi, pi] and every f32 within 64 ulp of 0, +-pi/2 and +-pi: where E_VSIN is measured"""
    lin = torch.linspace(-math.pi, math.pi, 2 ** 20, dtype=torch.float64).float()
    return torch.cat([lin, _neighbours([0.0, math.pi / 2, -math.pi / 2, math.pi, -math.pi], 64)])


def probe_range():
    """log-spaced |x| from 2^-30 to 2^20 on both signs, and the f32 neighbours (+- 2 ulp) of k pi for k up to 10^5"""
    mag = torch.exp2(torch.linspace(-30.0, 20.0, 2 ** 16, dtype=torch.float64)).float()
    kpi = (torch.arange(1, 100001, dtype=torch.float64) * math.pi).float().view(torch.int32)
    near = (kpi[:, None] + torch.arange(-2, 3, dtype=torch.int32)[None, :]).view(torch.float32).flatten()
    return torch.cat([mag, -mag, near, -near])


def probe_bound(x):
    """|sin_reduced(x) - sin64(x)| <= E_VSIN + 2^-22 + |k| 4e-14, k = round(x / 2 pi): the second reduction step's rounding (half an ulp of a
    value below 4) and the multiplication by 1 / 2 pi at its worst, and the residual of the two-constant 2 pi times k"""
    k = torch.round(x.double() / (2 * math.pi)).abs()
    return E_VSIN + 2.0 ** -22 + k * 4e-14
