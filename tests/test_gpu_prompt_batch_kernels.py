"""The four ragged prompt-side entries (include/indextts_hip.h: itts_tok_ctxpool_seq_forward, itts_tok_statspool_seq_forward,
itts_tok_gather_conv1d_seq_forward, itts_tok_gather_conv2d_seq_forward) on the GPU, through the C ABI.

* The two pools: BITWISE against the single-sequence entries (itts_tok_ctxpool_forward / itts_tok_statspool_forward, which
  tests/test_gpu_prompt_matrix.py holds to an f64 reference) run on each sequence's rows alone -- the sequence lengths of prompt_matrix.CTX_N in one
  ragged batch, those of POOL_N in a second, seg_len in {1, 100}, C in {1, 5}, seq_start with gaps whose rows hold NaN, the batch in both orders.
* The two gathers: BITWISE against the torch index expressions of `CAMPPlus._conv1d_rows` / `CAMPPlus._conv2d` per sequence (pure data movement),
  in two passes with the sequences of the other parity holding NaN: a tap that leaves its sequence returns NaN.
* Outputs are pre-filled with a NaN bit pattern and a sentinel tail: everything outside what an entry must write keeps its pattern.
* Bad arguments return ITTS_ERR_ARG before any launch."""
import pytest
import torch

from tests import prompt_matrix as PM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 4096
TAIL_BITS = 0x4B1D4B1D
NAN_BITS = 0x7FC5A5A5
ERR_ARG = 1
BATCHES = {"ctx_n": PM.CTX_N, "pool_n": PM.POOL_N}


@pytest.fixture(scope="module")
def eng():
    from indextts_amd import _lib, campplus
    return _lib, _lib.lib(), campplus._COps(DEV)


def _gapped(lens, lead=1, gap=2):
    """starts of sequences laid out with rows that belong to no sequence in front of, between and behind them -> (starts, total rows)"""
    starts, pos = [], lead
    for T in lens:
        starts.append(pos)
        pos += T + gap
    return starts, pos


def _i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def _frame(n):
    return torch.cat([torch.full((n,), NAN_BITS, dtype=torch.int32), torch.full((PAD,), TAIL_BITS, dtype=torch.int32)]).to(DEV)


def _bits(buf, n):
    host = buf.cpu()
    assert bool((host[n:] == TAIL_BITS).all()), f"{int((host[n:] != TAIL_BITS).sum())} words behind the output were overwritten"
    return host[:n]


def _seq_data(T, C, salt):
    g = torch.Generator().manual_seed(1000 * T + 10 * C + salt)
    off = torch.zeros(C)
    off[: min(C, 5)] = torch.tensor([0.0, 50.0, -200.0, 0.0, 1.0])[: min(C, 5)]
    return (torch.randn(T, C, generator=g) * torch.exp(1.5 * torch.randn(T, C, generator=g)) + off).contiguous()


def _pack(lens, C, salt):
    """-> (x [rows][C] with NaN in the gap rows, starts, rows, per-sequence data)"""
    starts, rows = _gapped(lens)
    x = torch.full((rows, C), PM.NAN)
    data = [_seq_data(T, C, salt) for T in lens]
    for s, d in zip(starts, data):
        x[s:s + d.shape[0]] = d
    return x, starts, rows, data


# ---- pools ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (1, 5))
@pytest.mark.parametrize("seg", (1, 100))
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_ctxpool_seq_has_the_bits_of_the_single_sequence_entry(eng, batch, seg, C):
    lib, L, ops = eng
    single = {}
    for lens in (list(BATCHES[batch]), list(BATCHES[batch])[::-1]):
        x, starts, rows, data = _pack(lens, C, 1)
        out, xd, sd, td = _frame(rows * C), x.to(DEV), _i32(starts), _i32(lens)      # (held: the launch reads them after the call returns)
        with lib.on_device(DEV):
            rc = L.itts_tok_ctxpool_seq_forward(lib.ptr(xd), lib.ptr(out), lib.ptr(sd), lib.ptr(td), len(lens), C, seg, lib.stream_ptr(DEV))
        assert rc == 0
        got = _bits(out, rows * C).view(rows, C)
        written = torch.zeros(rows, dtype=torch.bool)
        for T, s, d in zip(lens, starts, data):
            if T not in single:
                single[T] = ops.ctxpool(d.to(DEV), seg).cpu().view(torch.int32)
            assert torch.equal(got[s:s + T], single[T]), f"{batch} seg {seg} C {C}: sequence of {T} rows differs from the single-sequence entry"
            written[s:s + T] = True
        assert bool((got[~written] == NAN_BITS).all()), "rows outside every sequence were written"
        wrapped = ops.ctxpool_seq(xd, sd, td, seg).cpu().view(torch.int32)
        assert torch.equal(wrapped[written], got[written])


@pytest.mark.parametrize("C", (1, 5))
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_statspool_seq_has_the_bits_of_the_single_sequence_entry(eng, batch, C):
    lib, L, ops = eng
    single = {}
    for lens in (list(BATCHES[batch]), list(BATCHES[batch])[::-1]):
        x, starts, rows, data = _pack(lens, C, 2)
        out, xd, sd, td = _frame(len(lens) * 2 * C), x.to(DEV), _i32(starts), _i32(lens)
        with lib.on_device(DEV):
            rc = L.itts_tok_statspool_seq_forward(lib.ptr(xd), lib.ptr(out), lib.ptr(sd), lib.ptr(td), len(lens), C, lib.stream_ptr(DEV))
        assert rc == 0
        got = _bits(out, len(lens) * 2 * C).view(len(lens), 2 * C)
        for i, (T, d) in enumerate(zip(lens, data)):
            if T < 2:                                                   # no unbiased deviation: the entry leaves the row alone, the wrapper refuses
                assert bool((got[i] == NAN_BITS).all())
                continue
            if T not in single:
                single[T] = ops.statspool(d.to(DEV)).cpu().view(torch.int32)[0]
            assert torch.equal(got[i], single[T]), f"{batch} C {C}: sequence of {T} rows differs from the single-sequence entry"
        if min(lens) < 2:
            with pytest.raises(ValueError):
                ops.statspool_seq(xd, sd, td, lens)
        else:
            assert torch.equal(ops.statspool_seq(xd, sd, td, lens).cpu().view(torch.int32), got)


# ---- gathers ------------------------------------------------------------------------------------------------------------------------------------
def conv1d_index_rule(x, k, dilation, stride, pad):
    """the torch index expression of CAMPPlus._conv1d_rows on one sequence x [T][C] -> [T_out][k * C]"""
    T = x.shape[0]
    T_out = (T + 2 * pad - dilation * (k - 1) - 1) // stride + 1
    t = torch.arange(T_out)[:, None] * stride + torch.arange(k)[None, :] * dilation - pad
    idx = torch.where((t >= 0) & (t < T), t, torch.full_like(t, T))
    x_ext = torch.cat([x, torch.zeros(1, x.shape[1])], 0)
    return x_ext[idx.reshape(-1)].view(T_out, k * x.shape[1])


def conv2d_index_rule(x, F_in, T, ksize, stride_f):
    """the torch index expression of CAMPPlus._conv2d on one sequence x [F_in * T][C] -> [F_out * T][ksize * ksize * C]"""
    pad = (ksize - 1) // 2
    F_out = (F_in + 2 * pad - ksize) // stride_f + 1
    f = torch.arange(F_out)[:, None, None, None] * stride_f + torch.arange(ksize)[None, None, :, None] - pad
    t = torch.arange(T)[None, :, None, None] + torch.arange(ksize)[None, None, None, :] - pad
    ok = (f >= 0) & (f < F_in) & (t >= 0) & (t < T)
    idx = torch.where(ok, f * T + t, torch.full_like(f * T + t, F_in * T))
    x_ext = torch.cat([x, torch.zeros(1, x.shape[1])], 0)
    return x_ext[idx.reshape(-1)].view(F_out * T, ksize * ksize * x.shape[1])


GATHER1D_LENS = (1, 2, 4, 5, 63, 64, 65, 301)
GATHER1D_GEOMETRIES = ((5, 1, 2, 2), (3, 1, 1, 1), (3, 2, 1, 2), (1, 1, 1, 0))      # (k, dilation, stride, pad): TDNN, dense d = 1, dense d = 2, 1 x 1


@pytest.mark.parametrize("C", (1, 4, 5, 32))
@pytest.mark.parametrize("geom", GATHER1D_GEOMETRIES, ids=lambda g: "k%d-d%d-s%d-p%d" % g)
def test_gather_conv1d_seq_is_the_index_rule_per_sequence(eng, geom, C):
    lib, L, ops = eng
    k, dil, stride, pad = geom
    lens = list(GATHER1D_LENS)
    x, starts, rows, data = _pack(lens, C, 3)
    want = [conv1d_index_rule(d, k, dil, stride, pad) for d in data]
    lens_out = [w.shape[0] for w in want]
    tok_seq, tok_t, dstart, _ = PM._tables(lens_out)
    n_dst = int(sum(lens_out))
    seq_of_src = torch.full((rows,), -1, dtype=torch.long)
    for i, (s, T) in enumerate(zip(starts, lens)):
        seq_of_src[s:s + T] = i
    tsd, ttd, sd, td = tok_seq.to(DEV), tok_t.to(DEV), _i32(starts), _i32(lens)
    for parity in (0, 1):
        # the sequences of the other parity (and the gap rows) hold NaN: a tap that leaves its sequence shows; their own outputs may be anything
        xp = torch.where(((seq_of_src % 2 == parity) & (seq_of_src >= 0))[:, None], x, torch.full((), PM.NAN)).to(DEV)
        out = _frame(n_dst * k * C)
        with lib.on_device(DEV):
            rc = L.itts_tok_gather_conv1d_seq_forward(lib.ptr(xp), lib.ptr(out), lib.ptr(tsd), lib.ptr(ttd), lib.ptr(sd), lib.ptr(td), n_dst, C, k, dil,
                                                      stride, pad, lib.stream_ptr(DEV))
        assert rc == 0
        got = _bits(out, n_dst * k * C).view(n_dst, k * C)
        for i in range(parity, len(lens), 2):
            o = int(dstart[i])
            assert torch.equal(got[o:o + lens_out[i]], want[i].contiguous().view(torch.int32)), \
                f"k {k} dilation {dil} stride {stride} pad {pad} C {C}: sequence of {lens[i]} rows differs from the index rule"
    col = ops.gather_conv1d_seq(x.to(DEV), tsd, ttd, n_dst, sd, td, k, dilation=dil, stride=stride, pad=pad)
    assert torch.equal(col.cpu().view(torch.int32), torch.cat(want, 0).contiguous().view(torch.int32))


GATHER2D_T = (1, 2, 3, 17)


@pytest.mark.parametrize("ksize", (1, 3))
@pytest.mark.parametrize("stride_f", (1, 2))
@pytest.mark.parametrize("F_in", (1, 2, 5, 8))
def test_gather_conv2d_seq_is_the_index_rule_per_sequence(eng, F_in, stride_f, ksize):
    lib, L, ops = eng
    lens = list(GATHER2D_T)
    starts, rows = _gapped(lens)
    pad = (ksize - 1) // 2
    F_out = (F_in + 2 * pad - ksize) // stride_f + 1
    kk = ksize * ksize
    sd, td = _i32(starts), _i32(lens)
    for C in (1, 4, 5):
        data = [_seq_data(F_in * T, C, 4) for T in lens]                 # a sequence's rows (f, t) at f * T + t
        want = [conv2d_index_rule(d, F_in, T, ksize, stride_f) for d, T in zip(data, lens)]
        for parity in (0, 1):
            x = torch.full((F_in * rows, C), PM.NAN)
            for i in range(parity, len(lens), 2):
                x[F_in * starts[i]: F_in * (starts[i] + lens[i])] = data[i]
            out, xd = _frame(F_out * rows * kk * C), x.to(DEV)
            with lib.on_device(DEV):
                rc = L.itts_tok_gather_conv2d_seq_forward(lib.ptr(xd), lib.ptr(out), lib.ptr(sd), lib.ptr(td), len(lens), F_in, C, ksize, stride_f,
                                                          lib.stream_ptr(DEV))
            assert rc == 0
            got = _bits(out, F_out * rows * kk * C).view(F_out * rows, kk * C)
            written = torch.zeros(F_out * rows, dtype=torch.bool)
            for i, T in enumerate(lens):
                o = F_out * starts[i]
                written[o:o + F_out * T] = True
                if i % 2 == parity:
                    assert torch.equal(got[o:o + F_out * T], want[i].contiguous().view(torch.int32)), \
                        f"F_in {F_in} stride_f {stride_f} ksize {ksize} C {C}: sequence of {T} frames differs from the index rule"
            assert bool((got[~written] == NAN_BITS).all()), "rows outside every sequence's output block were written"
        # the wrapper, sequences packed back to back
        _, _, pstart, pT = PM._tables(lens)
        xp = torch.cat(data, 0)
        col, fo = ops.gather_conv2d_seq(xp.to(DEV), pstart.to(DEV), pT.to(DEV), int(sum(lens)), F_in, ksize=ksize, stride_f=stride_f)
        assert fo == F_out and torch.equal(col.cpu().view(torch.int32), torch.cat(want, 0).contiguous().view(torch.int32))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_err_arg_before_any_launch(eng):
    lib, L, ops = eng
    x = torch.ones(64, 4, device=DEV)
    tab = _i32([0])
    T = _i32([4])
    out = _frame(1024)
    p, st = lib.ptr, lib.stream_ptr(DEV)
    with lib.on_device(DEV):
        calls = [
            lambda: L.itts_tok_ctxpool_seq_forward(None, p(out), p(tab), p(T), 1, 4, 100, st),
            lambda: L.itts_tok_ctxpool_seq_forward(p(x), None, p(tab), p(T), 1, 4, 100, st),
            lambda: L.itts_tok_ctxpool_seq_forward(p(x), p(out), None, p(T), 1, 4, 100, st),
            lambda: L.itts_tok_ctxpool_seq_forward(p(x), p(out), p(tab), None, 1, 4, 100, st),
            lambda: L.itts_tok_ctxpool_seq_forward(p(x), p(out), p(tab), p(T), 0, 4, 100, st),
            lambda: L.itts_tok_ctxpool_seq_forward(p(x), p(out), p(tab), p(T), 1, 0, 100, st),
            lambda: L.itts_tok_ctxpool_seq_forward(p(x), p(out), p(tab), p(T), 1, 4, 0, st),
            lambda: L.itts_tok_statspool_seq_forward(None, p(out), p(tab), p(T), 1, 4, st),
            lambda: L.itts_tok_statspool_seq_forward(p(x), None, p(tab), p(T), 1, 4, st),
            lambda: L.itts_tok_statspool_seq_forward(p(x), p(out), None, p(T), 1, 4, st),
            lambda: L.itts_tok_statspool_seq_forward(p(x), p(out), p(tab), None, 1, 4, st),
            lambda: L.itts_tok_statspool_seq_forward(p(x), p(out), p(tab), p(T), 0, 4, st),
            lambda: L.itts_tok_statspool_seq_forward(p(x), p(out), p(tab), p(T), 1, 0, st),
            lambda: L.itts_tok_gather_conv1d_seq_forward(None, p(out), p(tab), p(tab), p(tab), p(T), 1, 4, 3, 1, 1, 1, st),
            lambda: L.itts_tok_gather_conv1d_seq_forward(p(x), None, p(tab), p(tab), p(tab), p(T), 1, 4, 3, 1, 1, 1, st),
            lambda: L.itts_tok_gather_conv1d_seq_forward(p(x), p(out), None, p(tab), p(tab), p(T), 1, 4, 3, 1, 1, 1, st),
            lambda: L.itts_tok_gather_conv1d_seq_forward(p(x), p(out), p(tab), None, p(tab), p(T), 1, 4, 3, 1, 1, 1, st),
            lambda: L.itts_tok_gather_conv1d_seq_forward(p(x), p(out), p(tab), p(tab), None, p(T), 1, 4, 3, 1, 1, 1, st),
            lambda: L.itts_tok_gather_conv1d_seq_forward(p(x), p(out), p(tab), p(tab), p(tab), None, 1, 4, 3, 1, 1, 1, st),
            lambda: L.itts_tok_gather_conv1d_seq_forward(p(x), p(out), p(tab), p(tab), p(tab), p(T), 1, 0, 3, 1, 1, 1, st),
            lambda: L.itts_tok_gather_conv1d_seq_forward(p(x), p(out), p(tab), p(tab), p(tab), p(T), 1, 4, 0, 1, 1, 1, st),
            lambda: L.itts_tok_gather_conv2d_seq_forward(None, p(out), p(tab), p(T), 1, 2, 4, 3, 1, st),
            lambda: L.itts_tok_gather_conv2d_seq_forward(p(x), None, p(tab), p(T), 1, 2, 4, 3, 1, st),
            lambda: L.itts_tok_gather_conv2d_seq_forward(p(x), p(out), None, p(T), 1, 2, 4, 3, 1, st),
            lambda: L.itts_tok_gather_conv2d_seq_forward(p(x), p(out), p(tab), None, 1, 2, 4, 3, 1, st),
            lambda: L.itts_tok_gather_conv2d_seq_forward(p(x), p(out), p(tab), p(T), 0, 2, 4, 3, 1, st),
            lambda: L.itts_tok_gather_conv2d_seq_forward(p(x), p(out), p(tab), p(T), 1, 2, 0, 3, 1, st),
            lambda: L.itts_tok_gather_conv2d_seq_forward(p(x), p(out), p(tab), p(T), 1, 2, 4, 2, 1, st),
        ]
        for i, call in enumerate(calls):
            assert call() == ERR_ARG, f"call {i} was not refused"
            assert L.itts_last_error()
    torch.cuda.synchronize()
    host = out.cpu()
    assert bool((host[:1024] == NAN_BITS).all()) and bool((host[1024:] == TAIL_BITS).all()), "a refused call wrote to its output"
