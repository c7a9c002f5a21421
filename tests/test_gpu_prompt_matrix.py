"""GPU: the prompt-side f32 kernels -- codec_kernels.hip, audio_kernels.hip (framed spectrum, resampler, column normalisation), the LayerNorm behind
itts_layernorm_forward -- through the unit entries of the C ABI, against an f64 reference at their own edges (tests/prompt_matrix.py: the cases,
the instance each is meant for, the operands, the references, the normalisers, the comparisons; tests/test_prompt_matrix_host.py holds the
premises).  Every launch of every case runs once:

  exact operands: the output equals the f64 result BITWISE (LayerNorm on constant rows, attention one-hot, the convs, the copy kernel, affine,
  scale_residual, ReLU, vq_project, the resampler on unit impulses, the VQ search on tied scores, attnstats one-hot);
  uniform operands: within 2 ulp of the f64 quotient;
  wide-range operands: within 4 E of the f64 result, E the plain-f32 CPU evaluation's own error under the same normaliser, computed in this run;
  canaries: the output is pre-filled with a NaN bit pattern and followed by 4096 sentinel words -- no valid element keeps the pattern, everything
  outside (columns past C under ld_out > C, rows in the gaps seq_start leaves, the output row stride's slack, rows of sequences whose neighbours
  hold NaN in the other pass) keeps it, the tail keeps its sentinel.  The in-place ops run inside such a frame too;
  refusals: ITTS_ERR_ARG with a message, the framed output untouched (each returns before any launch: read in the source of its entry).

The in-place ops go through the wrappers the models use (codec._TokOps, cond._Ops, campplus._COps), the column normalisation through
audio._colnorm, the plain resampler shape also through audio.Resample, every LayerNorm launch also through gpt.layernorm and every frame-major
spectrum also through audio._fbank (bitwise equal to the framed call); the other wrappers allocate their own outputs, which cannot carry a
canary, so those ops are called through _lib.lib().  The fused partial / bias flags of ln_kernel are not reachable through
itts_layernorm_forward and stay with tests/test_gpu_gpt.py.

One finding when the matrix first ran: LayerNorm on constant rows did not return beta at D = 192 (ln_small_kernel<3>) -- the third 64-element
chunk of every row came out 1e-5 off, the first two exact.  hipcc's default contraction had folded the mean's multiplication by 1 / D into that
chunk's subtraction alone (fma(-sum, 1 / D, x)), so equal inputs of one row left the kernel different.  ln_small_kernel and ln_generic_kernel now
round the mean once, as ln_row always did.

No pointwise op needed a per-function constant: the device's expf / erff / tanhf / log1pf stayed inside 4 E of the host's (table below).

The per-instance table is printed by test_every_kernel_was_hit (run with -s); the limits are measured on the reference side, never fitted to it.
As measured on an MI355X (gfx950) when the matrix was written, 2026-10-20 (every exact case bitwise equal, every canary intact):

    instance                           launches   largest error / limit
    ln_kernel<1>/wpb1                        24   0.1896
    ln_kernel<1>/wpb4                         4   0.1333
    ln_kernel<2>/wpb1                        24   0.1646
    ln_kernel<2>/wpb4                         4   0.1476
    ln_kernel<3>/wpb1                        24   0.1778
    ln_kernel<3>/wpb4                         4   0.1684
    ln_kernel<4>/wpb1                        24   0.1890
    ln_kernel<4>/wpb4                         4   0.1640
    ln_kernel<5>/wpb1                        24   0.1845
    ln_kernel<5>/wpb4                         4   0.1678
    ln_kernel<6>/wpb1                        24   0.1790
    ln_kernel<6>/wpb4                         4   0.1828
    ln_kernel<8>/wpb1                        24   0.1700
    ln_kernel<8>/wpb4                         4   0.2141
    ln_small_kernel<1>                       28   0.1453
    ln_small_kernel<2>                       28   0.1448
    ln_small_kernel<3>                       28   0.1667
    ln_small_kernel<5>                       28   0.1534
    ln_small_kernel<6>                       28   0.1688
    ln_small_kernel<10>                      28   0.1899
    ln_small_kernel<14>                      28   0.2043
    ln_generic_kernel                        98   0.1898
    attn_generic_kernel<16>                  30   0.0892
    attn_generic_kernel<16>/relkey            9   0.0787
    attn_generic_kernel<32>                  30   0.1053
    attn_generic_kernel<32>/relkey           13   0.0914
    dwconv_kernel/same                       16   0.1989
    dwconv_kernel/causal                     16   0.2500
    glu_kernel/mode0                          6   0.2500
    glu_kernel/mode1                          6   0.2365
    act_kernel/mode0                          7   -
    act_kernel/mode1                          6   0.2066
    act_kernel/mode2                          6   0.1718
    attnstats_kernel/none                    14   0.1094
    attnstats_kernel/const                   14   0.0953
    attnstats_kernel/onehot                   7   -
    attnstats_kernel/wide                     7   0.1777
    colnorm_kernel/mode0                      6   0.1099
    colnorm_kernel/mode1                     10   0.1316
    affine_act_kernel                        48   0.1467
    ctxpool_kernel                          132   0.1951
    fbank_kernel                             30   0.2973
    gate_kernel                               6   0.2754
    gather_conv_kernel                        4   -
    gelu_erf_kernel                           6   0.2500
    groupnorm1_mish_kernel                    3   0.2061
    l2norm_kernel                             5   0.2538
    resample_kernel                         138   0.2664
    scale_residual_kernel                    12   0.1386
    statspool_kernel                         12   0.1344
    vq_project_kernel                        10   0.2135
    vq_search_kernel                         36   -

    E per op: layernorm 2.703e-07, attention 3.455e-06, gelu 1.101e-07, glu 1.471e-07, act 1.589e-07, gate 1.390e-07, scale_residual
      1.016e-07, affine 9.977e-08, dwconv 4.518e-07, groupnorm_mish 8.508e-08, l2norm 2.175e-07, colnorm 2.305e-07, ctxpool 1.433e-07,
      statspool 2.082e-07, attnstats 3.067e-07, vq_project 2.448e-07, resample 2.840e-07, fbank 1.369e-06
    E per fbank case: kaldi 2.538e-07, mel 4.757e-07, n1024-m100 1.369e-06, n2048 2.021e-07, n512-reflect 1.425e-07, n64-fl2 1.941e-07,
      n64-hop1 4.911e-08
"""
import collections
import ctypes as C

import pytest
import torch

from tests import prompt_matrix as PM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 4096
TAIL_BITS = 0x4B1D4B1D                                                              # behind the output: a finite f32 bit pattern
NAN_BITS = 0x7FC5A5A5                                                               # a quiet NaN with a payload
IDX_FILL, IDX_TAIL = -0x5A5A5A5A5A5A5A5B, 0x4B1D4B1D4B1D4B1D                        # the same for the int64 indices of the VQ search
ERR_ARG = 1

HIT = collections.defaultdict(int)            # instance -> launches that ran on it
RATIO = collections.defaultdict(float)        # instance -> largest error / limit over its wide launches
INPLACE = ("gelu", "act", "gate", "scale_residual", "l2norm", "groupnorm_mish")


@pytest.fixture(scope="module")
def eng():
    from indextts_amd import _lib, audio, campplus, gpt
    E = collections.namedtuple("E", "lib L ops audio gpt")
    return E(_lib, _lib.lib(), campplus._COps(DEV), audio, gpt)                     # _COps: _TokOps + cond._Ops + the CAMPPlus ops


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _framed(valid, body=None, dtype=torch.int32, fill=NAN_BITS, tail=TAIL_BITS):
    """A device buffer of valid.numel() + PAD words: the fill pattern (`body` bits where valid, for the in-place ops), then the tail sentinel."""
    n = valid.numel()
    bits = torch.full((n,), fill, dtype=dtype)
    if body is not None:
        bits = torch.where(valid.flatten(), body.contiguous().view(dtype).flatten(), bits)
    return torch.cat([bits, torch.full((PAD,), tail, dtype=dtype)]).to(DEV)


def _read_back(buf, lch, dtype=torch.int32, fill=NAN_BITS, tail=TAIL_BITS):
    n = lch.valid.numel()
    host = buf.cpu()
    assert bool((host[n:] == tail).all()), f"{int((host[n:] != tail).sum())} words behind the output were overwritten"
    bits = host[:n].view(lch.valid.shape)
    keep = ~lch.valid if lch.ignore is None else ~lch.valid & ~lch.ignore
    assert bool((bits[keep] == fill).all()), f"{int((bits[keep] != fill).sum())} elements outside what the op writes were written"
    assert not bool((bits[lch.valid] == fill).any()), f"{int((bits[lch.valid] == fill).sum())} of {int(lch.valid.sum())} valid elements were never written"
    return bits


def _call(eng, c, a, out):
    """One engine call of the op on device operands; out: the f32 (int64: vq_search) view of the framed buffer, shaped like the launch's ref."""
    lib, L, p = eng.lib, eng.L, lib_ptr
    st = eng.lib.stream_ptr(torch.device(DEV))
    op = c.op
    with eng.lib.on_device(torch.device(DEV)):
        if op == "layernorm":
            rows, D = a["x"].shape
            x, g, b, g2, b2 = (_d(a[k]) for k in ("x", "g", "b", "g2", "b2"))
            rc = L.itts_layernorm_forward(p(x), p(g), p(b), p(g2), p(b2), p(out), rows, D, a["eps"], st)
            if rc == 0:
                assert torch.equal(eng.gpt.layernorm(x, g, b, g2, b2, a["eps"]).view(torch.int32), out.view(torch.int32)), "gpt.layernorm differs from the framed call"
        elif op == "attention":
            q, k, v, ks, kl = (_d(a[key]) for key in ("q", "k", "v", "kstart", "klen"))
            if a.get("emb") is None:
                rc = L.itts_attention_forward(p(q), p(k), p(v), p(out), p(ks), p(kl), q.shape[0], a["H"], a["dq"], a["dv"], a["scale"], st)
            else:
                qp, emb = _d(a["qpos"]), _d(a["emb"])
                rc = L.itts_attention_relkey_forward(p(q), p(k), p(v), p(out), p(ks), p(kl), p(qp), p(emb), a["left"], a["right"], q.shape[0], a["H"],
                                                     a["dq"], a["dv"], a["scale"], st)
        elif op == "gelu":
            eng.ops.gelu_(out); rc = 0
        elif op == "act":
            eng.ops.act_(out, a["mode"]); rc = 0
        elif op == "gate":
            eng.ops.gate_(out, _d(a["g"])); rc = 0
        elif op == "scale_residual":
            eng.ops.scale_residual_(out, _d(a["y"]), _d(a["gamma"])); rc = 0
        elif op == "l2norm":
            eng.ops.l2norm_(out, _d(a["gamma"]), a["scale"]); rc = 0
        elif op == "groupnorm_mish":
            eng.ops.groupnorm_mish_(out, _d(a["gamma"]), _d(a["beta"]), _d(a["seq_start"]), _d(a["seq_T"]), a["eps"]); rc = 0
        elif op == "glu":
            x = _d(a["x"])
            rc = L.itts_tok_glu_forward(p(x), p(out), x.shape[0], a["C"], a["mode"], st)
        elif op == "affine":
            x, sc, sh = _d(a["x"]), _d(a["scale"]), _d(a["shift"])
            rc = L.itts_tok_affine_forward(p(x), a["ld"], p(sc), p(sh), p(out), x.shape[0], a["C"], a["relu"], st)
        elif op == "dwconv":
            x, w, b, ts, tt, sT = (_d(a[key]) for key in ("x", "w", "b", "tok_seq", "tok_t", "seq_T"))
            fn = L.itts_tok_dwconv_causal_forward if a["causal"] else L.itts_tok_dwconv_forward
            rc = fn(p(x), p(w), p(b), p(out), p(ts), p(tt), p(sT), x.shape[0], x.shape[1], a["k"], st)
        elif op == "gather_conv":
            x, ts, tt, ss, sT, dT = (_d(a[key]) for key in ("x", "tok_seq", "tok_t", "src_start", "src_T", "dst_T"))
            rc = L.itts_tok_gather_conv_forward(p(x), p(out), p(ts), p(tt), p(ss), p(sT), p(dT), ts.numel(), a["C"], a["k"], st)
        elif op == "colnorm":
            eng.audio._colnorm(_d(a["x"]), out, a["mode"], a["ddof"], a["eps"]); rc = 0
        elif op == "ctxpool":
            x = _d(a["x"])
            rc = L.itts_tok_ctxpool_forward(p(x), p(out), x.shape[0], x.shape[1], a["seg_len"], st)
        elif op == "statspool":
            x = _d(a["x"])
            rc = L.itts_tok_statspool_forward(p(x), p(out), x.shape[0], x.shape[1], st)
        elif op == "attnstats":
            x, lg = _d(a["x"]), _d(a["logit"])
            rc = L.itts_tok_attnstats_forward(p(x), p(lg), p(out), x.shape[0], x.shape[1], a["eps"], st)
        elif op == "vq_project":
            codes, cb, w, bias = (_d(a[key]) for key in ("codes", "codebook", "w", "bias"))
            rc = L.itts_vq_project_forward(p(codes), p(cb), p(w), p(bias), p(out), codes.numel(), a["K"], a["cd"], a["H"], st)
        elif op == "vq_search":
            h, w, b, cb, c2 = (_d(a[key]) for key in ("h", "w_in", "b_in", "cb_norm", "cb_sq"))
            rc = L.itts_vq_search_forward(p(h), p(w), p(b), p(cb), p(c2), p(out), h.shape[0], a["H"], a["K"], a["cd"], st)
        elif op == "resample":
            x, kern = _d(a["x"]), _d(a["kernel"])
            rc = L.itts_resample_forward(p(x), p(kern), p(out), a["B"], a["L_in"], a["x_stride"], a["L_out"], a["y_stride"], a["orig"], a["new"],
                                         a["width"], st)
        elif op == "fbank":
            cfg = eng.lib.FbankConfig(frame_length=a["FL"], hop=a["hop"], n_fft=a["n_fft"], n_mels=a["n_mels"], pad=a["pad"], remove_dc=a["remove_dc"],
                                      power=a["power"], take_log=a["take_log"], layout=a["layout"], preemphasis=a["preemph"], mag_eps=a["mag_eps"],
                                      floor=a["floor"], scale=a["scale"])
            wave, win, tw, mel = (_d(a[key]) for key in ("wave", "window", "twiddle", "mel"))
            assert L.itts_fbank_frames(C.byref(cfg), a["n_samples"]) == PM.fbank_frames(a["FL"], a["hop"], a["pad"], a["n_samples"])
            rc = L.itts_fbank_forward(p(wave), a["B"], a["n_samples"], a["wave_stride"], C.byref(cfg), p(win), p(tw), p(mel), p(out), a["ld_out"],
                                      a["out_stride"], st)
            if rc == 0 and a["layout"] == 0:                            # the wrapper's own launch (tight strides) returns the same bits
                frames = PM.fbank_frames(a["FL"], a["hop"], a["pad"], a["n_samples"])
                if frames:
                    y = eng.audio._fbank(wave[:, :a["n_samples"]].contiguous(), cfg, win, tw, mel)
                    mine = out[:, :frames * a["ld_out"]].view(a["B"], frames, a["ld_out"])[:, :, :a["n_mels"]]
                    assert torch.equal(y.view(torch.int32), mine.contiguous().view(torch.int32)), "audio._fbank differs from the framed call"
        else:
            raise KeyError(op)
    return rc


def lib_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _run(eng, c, lch):
    """One launch into the canary-framed buffer -> the output on the host, shaped like lch.ref."""
    if c.op == "vq_search":
        buf = _framed(lch.valid, dtype=torch.int64, fill=IDX_FILL, tail=IDX_TAIL)
        out = buf[:lch.valid.numel()]
        eng.lib.check(_call(eng, c, lch.args, out), c.op)
        return _read_back(buf, lch, torch.int64, IDX_FILL, IDX_TAIL)
    buf = _framed(lch.valid, lch.args["x"] if c.op in INPLACE else None)
    out = buf[:lch.valid.numel()].view(torch.float32).view(lch.valid.shape)
    eng.lib.check(_call(eng, c, lch.args, out), c.op)
    return _read_back(buf, lch).view(torch.float32)


@pytest.mark.parametrize("c", PM.CASES, ids=PM.case_id)
def test_case_vs_f64(c, eng):
    fails = []
    for lch in PM.launches(c):
        out = _run(eng, c, lch)
        st = {}
        bad = PM.check(c, lch, out, st)
        inst = PM.instances_of(c)
        if c.op == "layernorm":
            inst = [PM.ln_instance(lch.args["x"].shape[1], lch.args["x"].shape[0], lch.args["g2"] is not None)]
        for i in inst:
            HIT[i] += 1
            RATIO[i] = max(RATIO[i], st.get("ratio", 0.0))
        if "ratio" in st:
            print(f"{PM.case_id(c)} {lch.label}: largest error / limit = {st['ratio']:.4f} (E = {st['E']:.3e})")
        fails += [f"{lch.label}: {b}" for b in bad]
    assert not fails, "\n".join(fails[:12])


def test_relu_past_one_grid_stride_pass(eng):
    """act_kernel's grid is capped at 65536 * 8 blocks: one more element count than a single pass of it, generated and checked on the device."""
    n = PM.BIG_RELU
    i = torch.arange(n, dtype=torch.int32, device=DEV)
    x = torch.cat([((i % 17) - 8).float(), torch.full((PAD,), 7.0, device=DEV)])
    want = x.clamp(min=0)
    eng.ops.act_(x[:n], 0)
    torch.cuda.synchronize()
    assert torch.equal(x, want)
    HIT["act_kernel/mode0"] += 1


def _refused(eng, call):
    buf = _framed(torch.ones(4096, dtype=torch.bool))
    with eng.lib.on_device(torch.device(DEV)):
        rc = call(lib_ptr(buf))
    torch.cuda.synchronize()
    msg = eng.L.itts_last_error().decode(errors="replace")
    assert rc == ERR_ARG and msg, (rc, msg)
    host = buf.cpu()
    assert bool((host[:4096] == NAN_BITS).all()) and bool((host[4096:] == TAIL_BITS).all()), "a refused call wrote its output"
    return msg


def test_refusals_leave_the_output_untouched(eng):
    L, p = eng.L, lib_ptr
    st = eng.lib.stream_ptr(torch.device(DEV))
    f = torch.ones(4096, device=DEV)
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    for D, second in PM.LN_REFUSALS:                                    # launch_ln / launch_ln_small_t / launch_ln_t: the width switch comes first
        g2 = p(f) if second else None
        assert "layernorm" in _refused(eng, lambda o: L.itts_layernorm_forward(p(f), p(f), p(f), g2, g2, o, 2, D, 1e-5, st))
    _refused(eng, lambda o: L.itts_vq_search_forward(p(f), p(f), p(f), p(f), p(f), o, 2, 8, 4, 17, st))                       # cd = 17
    for r in PM.ATTN_REFUSALS:                                          # attention_launch checks both before its n_q test
        if "left" in r:
            _refused(eng, lambda o: L.itts_attention_relkey_forward(p(f), p(f), p(f), o, p(i32), p(i32), p(i32), p(f), r["left"], r["right"], 2, 1,
                                                                    r["dq"], r["dv"], 0.125, st))
        else:
            _refused(eng, lambda o: L.itts_attention_forward(p(f), p(f), p(f), o, p(i32), p(i32), 2, 1, r["dq"], r["dv"], 0.125, st))
    for k in (2, 4):                                                    # even k for the same-padded convs
        _refused(eng, lambda o: L.itts_tok_dwconv_forward(p(f), p(f), p(f), o, p(i32), p(i32), p(i32), 2, 4, k, st))
        _refused(eng, lambda o: L.itts_tok_gather_conv_forward(p(f), o, p(i32), p(i32), p(i32), p(i32), p(i32), 2, 4, k, st))
    _refused(eng, lambda o: L.itts_tok_gather_conv_forward(p(f), o, p(i32), p(i32), p(i32), p(i32), p(i32), 2, 6, 3, st))     # C % 4 != 0
    _refused(eng, lambda o: L.itts_tok_statspool_forward(p(f), o, 1, 4, st))                                                 # n = 1
    full = PM.resample_full(10, 3, 2)                                   # L_out beyond what the padded conv produces
    _refused(eng, lambda o: L.itts_resample_forward(p(f), p(f), o, 1, 10, 10, full + 1, full + 1, 3, 2, 10, st))
    _refused(eng, lambda o: L.itts_tok_colnorm_forward(p(f), o, 1, 4, 4, 1, 1, 0.0, st))                                      # mode 1 with n = ddof
    _refused(eng, lambda o: L.itts_tok_colnorm_forward(p(f), o, 2, 4, 3, 0, 0, 0.0, st))                                      # ld_out < C
    # the framed-spectrum entry: n_fft not a power of two, above 2048, reflect padding that needs more samples (all checked before the frame count)
    for n_fft, pad, n in ((96, 0, 400), (4096, 0, 8000), (512, 300, 300), (512, 301, 300)):
        cfg = eng.lib.FbankConfig(frame_length=min(n_fft, 64), hop=16, n_fft=n_fft, n_mels=4, pad=pad, remove_dc=0, power=2, take_log=0, layout=0,
                                  preemphasis=0.0, mag_eps=0.0, floor=0.0, scale=1.0)
        assert "fbank" in _refused(eng, lambda o: L.itts_fbank_forward(p(f), 1, n, n, C.byref(cfg), p(f), p(f), p(f), o, 4, 4096, st))


def test_plain_resample_through_the_wrapper(eng):
    """audio.Resample builds the same tap table and the same L_out = ceil(new L / orig) launch the matrix runs framed."""
    for c in [c for c in PM.CASES if c.op == "resample"]:
        p = PM.P(c)
        for lch in PM.launches(c, ("wide",)):
            a = lch.args
            if a["L_in"] == 1000 and a["L_out"] == -(-p["new"] * 1000 // p["orig"]):
                y = eng.audio.Resample(p["orig"], p["new"], device=DEV)(_d(a["x"][:, :1000])).cpu()
                assert PM.check(c, lch._replace(ref=lch.ref[:, :a["L_out"]], norm=lch.norm[:, :a["L_out"]], valid=lch.valid[:, :a["L_out"]]), y) == []


def test_docstring_table_names_every_instance():
    for i in PM.ALL_INSTANCES:
        assert f"    {i} " in __doc__, i


def test_every_kernel_was_hit():
    want = list(PM.ALL_INSTANCES)
    print()
    print(f"    {'instance':<34}{'launches':>9}   largest error / limit")
    for i in want:
        print(f"    {i:<34}{HIT[i]:>9}   {RATIO[i]:.4f}" if RATIO[i] else f"    {i:<34}{HIT[i]:>9}   -")
    print("    E per op: " + ", ".join(f"{op} {PM.baseline_E(op):.3e}" for op in PM.OPS if PM.baseline_E(op) > 0))
    missing = [i for i in want if HIT[i] == 0]
    assert not missing, f"no launch ran on {missing}"
