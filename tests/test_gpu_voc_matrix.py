"""GPU: every kernel behind the vocoder's conv and activation launchers, through the unit entries, against an f64 reference at its own edges
(tests/voc_matrix.py: the cases, the kernel each is meant for, the operands, the references, the bounds; tests/test_voc_matrix_host.py holds
the premises).  Per conv case (f32 MFMA conv at four co-tile heights, its transposed form, bf16 x 3, f16 x 3):

  the path: the options are set, the op runs once, and `itts_voc_last_path()` must name the kernel the case was built for;
  exact operands: the output equals the f64 convolution BITWISE;
  wide-range operands: (a) elementwise inside the derived first-order bound, (b) with at least 4096 outputs, RMS error at most 1.5 x that of a
  plain f32 accumulation on the CPU (plus the split emulation's error in the f16 x 3 mode);
  canaries: the output is pre-filled with a NaN bit pattern (under the accumulate epilogues: the accumulate buffer inside the rows, the
  pattern beyond them) and carries 4096 extra floats behind it -- no valid element keeps the pattern, every frame beyond a row's length does,
  the tail keeps its sentinel.

Per activation case (three f32 variants and the planes kernel; mild and wide parameter sets): the path, the stage-by-stage bound, the same
canaries; the planes kernel's three planes sum to an f32 value inside the bound, are bitwise the bf16 split of the aa_v2_vsin output and are
zeros beyond a row's length.  test_sin_reduced_probe measures the default kernels' sine on its own (E_VSIN in tests/voc_matrix.py).

The per-path table is printed by test_every_path_was_hit (run with -s); the bounds are derived, never fitted to it.  As measured on an MI355X
when the matrix was written (every exact case bitwise equal, every canary intact):

    path                  cases   largest error / bound   largest rms error / f32 baseline (limit 1.5)
    conv_f32_bm32            87   0.1109                  1.2409
    conv_f32_bm64            29   0.1437                  1.0654
    conv_f32_bm96            29   0.1034                  1.3756
    conv_f32_bm128           49   0.1376                  1.1925
    conv_x3_nh1              37   0.0275                  1.2788
    conv_x3_nh2              37   0.0283                  0.9710
    conv_h3_two_stage        26   0.0724                  0.7104
    conv_h3_win256x128       28   0.0151                  0.5960
    conv_h3_win192x192       28   0.0180                  0.7164
    conv_h3_win256x96        28   0.0164                  0.5526
    aa_v1_sinf               30   0.1624                  -
    aa_v2_sinf               30   0.1624                  -
    aa_v2_vsin               30   0.1619                  -
    aa_planes_vsin           30   0.2410                  -

    sin_reduced on [-pi, pi]: largest |y - sin64(x)| = 2.8392e-07 at x = 3.1416006 (E_VSIN = 5.6784e-07); out to |x| = 2^20 and at the
    neighbours of k pi, k <= 10^5: largest error / bound = 0.5344 at x = 46058.89

(341 of the 378 conv cases carry the rms criterion.  The largest rms ratios, 1.24 .. 1.38, all belong to cases with a single 32-channel
chunk and k <= 7 (32 -> 97 channels at k = 7 on the 96-row tile; 32 -> 96 at k = 3 on the x3 kernel); two opposite summation orders of the
CPU baseline itself differ by up to 1.25 x, and a lost plane shows as 3 x and more, tests/test_voc_matrix_host.py.)
"""
import collections

import pytest
import torch

from tests import voc_matrix as VM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 4096
TAIL_BITS = 0x4B1D4B1D                                                              # behind the output: a finite f32 bit pattern
NAN_BITS = 0x7FC5A5A5                                                               # a quiet NaN with a payload
TAIL16, NAN16 = 0x4B1D, 0x7FC5                                                      # the same for the bf16 planes

HIT = collections.defaultdict(int)            # path -> cases that ran on it
RATIO = collections.defaultdict(float)        # path -> largest error / bound
RMSR = collections.defaultdict(float)         # conv path -> largest rms error / rms error of the f32 baseline (limit: 1.5)


@pytest.fixture(scope="module")
def bv():
    from indextts_amd import bigvgan
    return bigvgan


@pytest.fixture(scope="module")
def packed(bv):
    """Packed weights on the device, shared by the cases of one (mode, C_in, C_out, k): packing is host work."""
    cache = {}

    def get(c, kind):
        key = (c.op,) + VM.weight_key(c) + (kind,)
        if key not in cache:
            w = VM.weights(VM.weight_key(c), kind)
            pack = {"f32": bv.pack_conv1d_weight, "x3": bv.pack_conv1d_x3_weight, "h3": bv.pack_conv1d_h3_weight,
                    "convT": lambda t: bv.pack_convT_weight(t, c.d)}[c.op]
            cache[key] = pack(w).to(DEV)
        return cache[key]
    return get


def _framed(n, body_bits):
    """An int32 device buffer of n + PAD elements: body_bits (a scalar or n values) then the tail sentinel."""
    buf = torch.empty(n + PAD, dtype=torch.int32, device=DEV)
    buf[:n] = body_bits
    buf[n:] = TAIL_BITS
    return buf


def _run_conv(bv, c, kind, wp):
    """One launch into the canary-framed buffer; returns the [B][Cout][T_out] block on the host and the path taken."""
    from indextts_amd import _lib
    o = VM.operands(c, kind)
    hb, hbb, hr, acc = VM.flags(c)
    To, valid = VM.t_out(c), VM.valid_mask(c)
    n = c.B * c.Cout * To
    body = torch.full((n,), NAN_BITS, dtype=torch.int32)
    if acc:
        body = torch.where(valid.flatten(), o.y0.contiguous().view(torch.int32).flatten(), body)
    buf = _framed(n, body.to(DEV))
    out = buf[:n].view(torch.float32).view(c.B, c.Cout, To)
    d = lambda t, on: t.to(DEV).contiguous() if on else None
    kw = dict(lens=list(c.lens) if c.lens is not None else None, len_mult=c.lm, out=out)
    with _lib.option_scope(**dict(c.opts)):
        if c.op == "convT":
            bv.conv_transpose1d(o.x.to(DEV), wp, d(o.bias, hb), c.Cout, c.k, c.d, bias_b=d(o.bias_b, hbb), **kw)
        else:
            fn = {"f32": bv.conv1d, "x3": bv.conv1d_x3, "h3": bv.conv1d_h3}[c.op]
            if c.op == "f32":
                kw["bias_b"] = d(o.bias_b, hbb)
            fn(o.x.to(DEV), wp, d(o.bias, hb), c.Cout, c.k, c.d, res=d(o.res, hr), acc_mode=acc, div=o.div, **kw)
        path = _lib.voc_last_path()
    host = buf.cpu()
    assert bool((host[n:] == TAIL_BITS).all()), f"{int((host[n:] != TAIL_BITS).sum())} floats behind the output were overwritten"
    bits = host[:n].view(c.B, c.Cout, To)
    assert bool((bits[~valid] == NAN_BITS).all()), f"{int((bits[~valid] != NAN_BITS).sum())} frames beyond a row's length were written"
    y = bits.view(torch.float32)
    assert not bool(torch.isnan(y[valid]).any()), f"{int(torch.isnan(y[valid]).sum())} of {int(valid.sum())} valid elements were never written"
    return y, path, o, valid


def _check_conv(bv, c, packed):
    y, path, o, valid = _run_conv(bv, c, "exact", packed(c, "exact"))
    assert path == c.path, f"meant for {c.path}, ran on {path}"
    HIT[path] += 1
    ref = VM.ref64(c, o)
    if not torch.equal(y.double()[valid], ref[valid]):
        bad = ((y.double() != ref) & valid).nonzero()
        raise AssertionError(f"{int(bad.shape[0])} of {int(valid.sum())} elements differ from the f64 result; first at {bad[0].tolist()}: "
                             f"{float(y[tuple(bad[0])])} vs {float(ref[tuple(bad[0])])}; rows {sorted(set(bad[:, 0].tolist()))[:8]} "
                             f"channels {sorted(set(bad[:, 1].tolist()))[:8]} frames {sorted(set(bad[:, 2].tolist()))[:8]}")
    y, path, o, valid = _run_conv(bv, c, "wide", packed(c, "wide"))
    assert path == c.path
    if not bool(valid.any()):
        return
    ref, bd = VM.ref64(c, o), VM.bound(c, o)
    ratio = float(((y.double() - ref).abs() / bd)[valid].max())
    RATIO[path] = max(RATIO[path], ratio)
    msg = f"{VM.conv_id(c)}: largest error / bound = {ratio:.4f}"
    rr = None
    if VM.carries_rms(c):
        limit = VM.rms_limit(c, o, ref)
        rr = VM.rms(y.double() - ref, valid) / (limit / VM.RMS_MARGIN)
        RMSR[path] = max(RMSR[path], rr)
        msg += f", rms error / f32 baseline = {rr:.4f}"
    print(msg)
    assert ratio <= 1.0, ratio
    assert rr is None or rr <= VM.RMS_MARGIN, rr


@pytest.mark.parametrize("c", VM.CONV_CASES, ids=VM.conv_id)
def test_conv_path_vs_f64(c, bv, packed):
    _check_conv(bv, c, packed)


def _run_act(bv, c, path=None):
    """One launch of the f32 activation into the canary-framed buffer -> ([B][C][T] on the host, path)."""
    from indextts_amd import _lib
    o = VM.act_operands(c)
    n = c.B * c.C * c.T
    buf = _framed(n, NAN_BITS)
    f = VM.O.default_filter()
    with _lib.option_scope(**dict(c.opts)):
        bv.anti_alias_activation(o.x.to(DEV), f, f, o.alpha, o.beta, lens=list(c.lens) if c.lens is not None else None, logscale=bool(c.logscale),
                                 len_mult=c.lm, out=buf[:n].view(torch.float32).view(c.B, c.C, c.T))
        path = _lib.voc_last_path()
    host = buf.cpu()
    valid = VM.act_valid(c)
    assert bool((host[n:] == TAIL_BITS).all()), "floats behind the output were overwritten"
    bits = host[:n].view(c.B, c.C, c.T)
    assert bool((bits[~valid] == NAN_BITS).all()), f"{int((bits[~valid] != NAN_BITS).sum())} frames beyond a row's length were written"
    y = bits.view(torch.float32)
    assert not bool(torch.isnan(y[valid]).any()), "valid elements were never written"
    return y, path


def _run_planes(bv, c):
    """One launch of the planes kernel into a canary-framed bf16 buffer -> ([3][B][T][C] int16 bit patterns on the host, path)."""
    from indextts_amd import _lib
    o = VM.act_operands(c)
    n = 3 * c.B * c.T * c.C
    buf = torch.empty(n + PAD, dtype=torch.int16, device=DEV)
    buf[:n] = NAN16
    buf[n:] = TAIL16
    f = VM.O.default_filter()
    with _lib.option_scope(**dict(c.opts)):
        bv.anti_alias_activation_planes(o.x.to(DEV), f, f, o.alpha, o.beta, lens=list(c.lens) if c.lens is not None else None,
                                        logscale=bool(c.logscale), len_mult=c.lm, out=buf[:n].view(torch.bfloat16).view(3, c.B, c.T, c.C))
        path = _lib.voc_last_path()
    host = buf.cpu()
    assert bool((host[n:] == TAIL16).all()), "elements behind the planes were overwritten"
    assert not bool((host[:n] == NAN16).any()), "plane elements were never written"
    return host[:n].view(3, c.B, c.T, c.C), path


def _check_act(bv, c):
    ref, bd, valid = VM.act_ref_bound(c)
    if c.path == "aa_planes_vsin":
        bits, path = _run_planes(bv, c)
        assert path == c.path, f"meant for {c.path}, ran on {path}"
        HIT[path] += 1
        vt = valid.permute(0, 2, 1)                                                  # [B][T][C]
        assert not bool(bits[:, ~vt].any()), "frames beyond a row's length are not zeros in all three planes"
        planes = bits.view(torch.bfloat16).double()
        tot = planes[0] + planes[1] + planes[2]                                      # exact in f64
        assert torch.equal(tot.float().double(), tot), "the three planes do not sum to an f32 value"
        y = tot.float().permute(0, 2, 1)
        two, p2 = _run_act(bv, c._replace(path="aa_v2_vsin"))                        # the two-kernel path on the same input
        assert p2 == "aa_v2_vsin"
        h, m, l = VM.split_x3(torch.where(valid, two, torch.zeros_like(two)).permute(0, 2, 1).contiguous())
        want = torch.stack([h, m, l]).bfloat16().view(torch.int16)
        assert torch.equal(bits, want), f"{int((bits != want).sum())} plane elements differ from the bf16 split of the aa_v2_vsin output"
    else:
        y, path = _run_act(bv, c)
        assert path == c.path, f"meant for {c.path}, ran on {path}"
        HIT[path] += 1
    if not bool(valid.any()):
        return
    ratio = float(((y.double() - ref).abs() / bd)[valid].max())
    RATIO[path] = max(RATIO[path], ratio)
    print(f"{VM.act_id(c)}: largest error / bound = {ratio:.4f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("c", VM.ACT_CASES, ids=VM.act_id)
def test_activation_path_vs_f64(c, bv):
    _check_act(bv, c)


def test_sin_reduced_probe(bv):
    """The default activation kernels' sine on its own, against an f64 sine: the largest absolute error on the grid across [-pi, pi] (E_VSIN is
    twice the value measured when the matrix was written, and the project allows at most 6e-6), and the reduction over the range it exists
    for: |x| from 2^-30 to 2^20 and the f32 neighbours of k pi up to k = 10^5."""
    x = VM.probe_grid()
    err = (bv.sin_reduced(x.to(DEV)).cpu().double() - torch.sin(x.double())).abs()
    i = int(err.argmax())
    print(f"sin_reduced on [-pi, pi]: largest |y - sin64(x)| = {float(err[i])!r} at x = {float(x[i])!r} ({x.numel()} points); "
          f"E_VSIN_MEASURED = {VM.E_VSIN_MEASURED!r}, E_VSIN = {VM.E_VSIN!r}")
    assert VM.E_VSIN <= VM.E_VSIN_CAP
    # the hardware function is deterministic; the 1e-6 relative slack is for the host's f64 sine, which may differ in its last bit
    assert float(err.max()) <= VM.E_VSIN_MEASURED * (1 + 1e-6), "the sine's error on the grid is above the value E_VSIN was doubled from"
    x = VM.probe_range()
    r = (bv.sin_reduced(x.to(DEV)).cpu().double() - torch.sin(x.double())).abs() / VM.probe_bound(x)
    i = int(r.argmax())
    print(f"sin_reduced out to 2^20: largest error / bound = {float(r[i]):.4f} at x = {float(x[i])!r}")
    assert float(r.max()) <= 1.0


def test_span_above_the_halo_is_an_engine_error(bv, packed):
    """(k - 1) * dilation above 64 comes back as an error from the f32 and the bf16 x 3 entries, never as a launch."""
    from indextts_amd import _lib
    for op, k, d in (("f32", 3, 33), ("f32", 5, 17), ("x3", 3, 33), ("x3", 11, 7)):
        c = VM.Conv(op, 1, 32, 33, 40, k, d, None, 1, "bias", (), "")
        with pytest.raises(_lib.HipEngineError, match="span|dilation"):
            _run_conv(bv, c, "exact", packed(c, "exact"))
    c = VM.Conv("x3", 1, 32, 33, 40, 1, 1, None, 1, "bias", (), "")
    with pytest.raises(_lib.HipEngineError):
        _run_conv(bv, c, "exact", packed(c, "exact"))                                  # k = 1 has no x3 kernel: refused, no fall-back
    torch.cuda.synchronize()


def test_path_list_is_the_checked_in_one():
    from indextts_amd import _lib
    assert _lib.voc_path_names() == VM.ALL_PATHS


def test_every_path_was_hit(bv, packed):
    """Every name of itts_voc_path_name ran in this process on a case of the matrix (a path whose cases were deselected runs its first case
    here), and the per-path table: cases, largest error / bound, and for the conv paths the largest rms error / f32 baseline (limit 1.5)."""
    from indextts_amd import _lib
    for p in VM.ALL_PATHS:
        if not HIT[p]:
            if p in VM.CONV_PATHS:
                _check_conv(bv, next(c for c in VM.CONV_CASES if c.path == p and VM.carries_rms(c)), packed)
            else:
                _check_act(bv, next(c for c in VM.ACT_CASES if c.path == p))
    names = _lib.voc_path_names()
    assert [p for p in names if not HIT[p]] == []
    print("path                  cases   largest error / bound   largest rms error / f32 baseline")
    for p in names:
        print(f"{p:<22}{HIT[p]:>5}   {RATIO[p]:<22.4f}  " + (f"{RMSR[p]:.4f}" if p in VM.CONV_PATHS else "-"))


def test_docstring_table_names_every_path():
    """The table of this file's docstring ("as measured on an MI355X when the matrix was written") has a row for every path the library lists."""
    from indextts_amd import _lib
    table = __doc__.split("when the matrix was written", 1)[1]
    assert [p for p in _lib.voc_path_names() if p not in table] == []
