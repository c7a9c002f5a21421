"""GPU: the two kernels behind `launch_attention` (attn_kernel at 4 / 8 / 16 waves with and without the beam row map, attn_prefill_mfma_kernel;
both cache precisions), through `itts_gpt_attention_forward`, against an f64 reference at their own edges (tests/attn_matrix.py: the cases, the
kernel each is meant for, the operands, the reference, the comparisons; tests/test_attn_matrix_host.py shows that those comparisons fail on
a reference with one defect).  Per case and attn_waves setting:

  a. the path: the options are set, the launch runs, and `itts_attention_last_path()` must name the kernel the case was built for (the
     default pick included: 16 waves up to 256 blocks, 8 above, 4 with several queries per sequence);
  b. one-hot operands, the target in turn at every edge of the window: the output equals the target's V row BITWISE;
  c. uniform operands: the mean of the window's V rows, i.e. a count of its keys;
  d. wide-range random operands: elementwise inside 4 x the error of torch's plain f32 evaluation of the same definition (+ one bf16 step
     of the output in the bf16 engine);
  canaries: keys no query may see hold V = 1e30 (finite: the MFMA kernel multiplies masked probabilities into V), cells behind the last
  written key and rows no table names hold NaN, the caches and the output sit between sentinel guards, the output is pre-filled with NaN:
  the guards keep their bits and no element of the output is NaN or Inf;
  the stream kernel's outputs at 4, 8 and 16 waves are bitwise equal.

The largest error / limit of the random family per path is printed by test_every_path_was_hit (run with -s); the limit is measured on the
reference side, never fitted to the kernels.  As measured on an MI355X when the matrix was written (every one-hot launch bitwise equal,
every canary intact, no kernel changed):

    streams f32,  4 / 8 / 16 waves             0.330      streams f32,  row map, 4 / 8 / 16 waves    0.251
    streams bf16, 4 / 8 / 16 waves             0.500      streams bf16, row map, 4 / 8 / 16 waves    0.499
    prefill MFMA f32                           0.618      prefill MFMA bf16                          0.494

(the bf16 stream kernel sits at the half step of its own output rounding.  Under 4 E + one bf16 step alone the bf16 MFMA kernel reached
1.482 in 4 of its 53 cases: its query and probabilities enter the matrix pipe as 16-bit hi + lo pairs; attn_matrix.hilo_term derives that
term, and with it the figure is the 0.494 above.)
"""
import collections
import ctypes as C

import pytest
import torch

from tests import attn_matrix as AM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024                                                                        # elements in front of and behind every buffer
GUARD_BITS = {torch.int32: 0x4B1D4B1D, torch.int16: 0x4B1D}                         # finite bit patterns
NAN_BITS = {torch.int32: 0x7FC5A5A5, torch.int16: 0x7FC5}                           # quiet NaNs with a payload (f32, bf16)

HIT = collections.defaultdict(int)            # path -> launches that ran on it
RATIO = collections.defaultdict(float)        # path -> largest error / limit of the random family


def _guarded(x, bf16):
    """Host f32 values -> a device buffer in the engine's dtype (as integers), GUARD sentinel elements on either side."""
    bits = (x.bfloat16().contiguous().view(torch.int16) if bf16 else x.contiguous().view(torch.int32)).flatten()
    buf = torch.empty(bits.numel() + 2 * GUARD, dtype=bits.dtype, device=DEV)
    buf[:GUARD] = GUARD_BITS[bits.dtype]
    buf[-GUARD:] = GUARD_BITS[bits.dtype]
    buf[GUARD:-GUARD] = bits.to(DEV)
    return buf


def _inner(buf):
    return C.c_void_p(buf.data_ptr() + GUARD * buf.element_size())


def _guards_intact(buf):
    s = GUARD_BITS[buf.dtype]
    return bool((buf[:GUARD] == s).all()) and bool((buf[-GUARD:] == s).all())


def _i32(x):
    return torch.as_tensor(x, dtype=torch.int32).contiguous().to(DEV) if x is not None else None


def _tables(c):
    m0, m1 = AM.row_maps(c.nseq, c.Tmax) if c.rmap else (None, None)
    return dict(pos=_i32([c.pos]), pad=_i32(c.pad), shift=_i32(c.shift), seq_map=_i32(c.seq_map), m0=_i32(m0), m1=_i32(m1),
                step=_i32([c.step]) if c.rmap else None)


def _launch(c, tab, q, kbuf, vbuf, waves):
    """One launch into a guarded, NaN-filled output; returns the [nseq][nq][D] block on the host in the engine's dtype, and the path taken."""
    from indextts_amd import _lib
    bf16 = c.prec == AM.PREC_BF16
    n = c.nseq * c.nq * AM.D
    out = torch.empty(n + 2 * GUARD, dtype=torch.int16 if bf16 else torch.int32, device=DEV)
    out[:GUARD] = GUARD_BITS[out.dtype]
    out[-GUARD:] = GUARD_BITS[out.dtype]
    out[GUARD:-GUARD] = NAN_BITS[out.dtype]
    with _lib.option_scope(attn_waves=waves, **dict(c.opts)):
        _lib.check(_lib.lib().itts_gpt_attention_forward(
            _lib.ptr(q), _inner(kbuf), _inner(vbuf), _inner(out), _lib.ptr(tab["pos"]), _lib.ptr(tab["pad"]), _lib.ptr(tab["shift"]),
            _lib.ptr(tab["seq_map"]), _lib.ptr(tab["m0"]), _lib.ptr(tab["m1"]), _lib.ptr(tab["step"]), c.nseq, AM.H, c.nq, c.Tmax, c.seq_mul,
            c.prec, _lib.stream_ptr(torch.device(DEV))), "itts_gpt_attention_forward")
        path = _lib.attention_last_path()
    host = out.cpu()
    assert _guards_intact(host), "the output's guards were overwritten"
    block = host[GUARD:-GUARD].view(torch.bfloat16 if bf16 else torch.float32).view(c.nseq, c.nq, AM.D)
    return block, path


def _check(c):
    bf16 = c.prec == AM.PREC_BF16
    tab = _tables(c)
    vkeep = {}
    for L in AM.launches(c):
        q = L.q.contiguous().to(DEV)
        kbuf = _guarded(L.k, bf16)
        if id(L.v) not in vkeep:
            vkeep = {id(L.v): _guarded(L.v, bf16)}
        vbuf = vkeep[id(L.v)]
        outs = []
        for waves in c.waves:
            out, path = _launch(c, tab, q, kbuf, vbuf, waves)
            assert path == AM.path_of(c, waves), f"attn_waves={waves}: meant for {AM.path_of(c, waves)}, ran on {path}"
            HIT[path] += 1
            if L.ratio:
                r = L.ratio(out)
                RATIO[path] = max(RATIO[path], r)
                print(f"{AM.case_id(c)} {path}: largest error / limit = {r:.4f}")
            fails = L.check(out)
            assert not fails, f"{L.label}, {path}: " + "; ".join(fails)
            outs.append(out)
        assert _guards_intact(kbuf) and _guards_intact(vbuf), f"{L.label}: the caches' guards were overwritten"
        if c.kind == "streams":
            ints = torch.int16 if bf16 else torch.int32
            for waves, o in zip(c.waves[1:], outs[1:]):
                assert torch.equal(o.view(ints), outs[0].view(ints)), f"{L.label}: attn_waves={waves} differs bitwise from attn_waves={c.waves[0]}"


@pytest.mark.parametrize("c", AM.CASES, ids=AM.case_id)
def test_attention_path_vs_f64(c):
    _check(c)


def test_entry_refuses_bad_arguments():
    from indextts_amd import _lib
    L = _lib.lib()
    q, k, v, o = (torch.zeros(2 * 8 * 64, device=DEV) for _ in range(4))       # one sequence, 2 heads, 8 keys
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    n, st = None, _lib.stream_ptr(torch.device(DEV))
    args = (("q", _lib.ptr(q)), ("k", _lib.ptr(k)), ("v", _lib.ptr(v)), ("out", _lib.ptr(o)), ("pos", _lib.ptr(i)), ("pad", n), ("shift", n),
            ("seq_map", n), ("m0", n), ("m1", n), ("step", n), ("nseq", 1), ("heads", 2), ("nq", 1), ("Tmax", 8), ("seq_mul", 1), ("prec", 0), ("st", st))
    ok = lambda **kw: L.itts_gpt_attention_forward(*[kw.get(name, dflt) for name, dflt in args])
    assert ok() == 0
    for bad in (dict(q=n), dict(k=n), dict(v=n), dict(out=n), dict(pos=n), dict(prec=2), dict(prec=-1), dict(nseq=0), dict(heads=0), dict(nq=0),
                dict(nq=65536), dict(Tmax=0), dict(seq_mul=-1), dict(m1=_lib.ptr(i)), dict(step=_lib.ptr(i)), dict(m0=_lib.ptr(i), m1=_lib.ptr(i))):
        assert ok(**bad) == _lib.ERR_ARG, bad
    torch.cuda.synchronize()


def test_path_list_is_the_checked_in_one():
    from indextts_amd import _lib
    assert _lib.attention_path_names() == AM.ALL_PATHS


def test_every_path_was_hit():
    """Every name of itts_attention_path_name ran in this process on a case of the matrix (a path whose cases were deselected runs its first
    case here), and the per-path table of the random family's largest error / limit."""
    from indextts_amd import _lib
    for p in AM.ALL_PATHS:
        if not HIT[p]:
            _check(next(c for c in AM.CASES if p in {AM.path_of(c, w) for w in c.waves}))
    names = _lib.attention_path_names()
    assert [p for p in names if not HIT[p]] == []
    print("path                      launches   largest error / limit")
    for p in names:
        print(f"{p:<26}{HIT[p]:>8}   {RATIO[p]:.4f}")
