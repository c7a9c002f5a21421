"""The prompt-side f32 kernel test matrix shared by tests/test_gpu_prompt_matrix.py (GPU) and tests/test_prompt_matrix_host.py (CPU): everything that
runs once per speaker prompt plus the step between the GPT codes and the decoder -- the 16 kernels of codec_kernels.hip, the three of
audio_kernels.hip and the LayerNorm behind itts_layernorm_forward -- at the edges of each kernel, through the unit entries of the C ABI
(include/indextts_hip.h).  The case tables, the kernel or template instance each case is meant for (`instances_of`, the launchers' dispatch rules
restated in one place), the operands, f64 references written from the definitions in the header and the kernel comments, the normalisers and the
comparisons both files apply.  No GPU import.

Every op is one `evaluate(args, dtype, mutant)` written from its definition: evaluated in f64 it is the reference, in plain f32 torch it is the
baseline the limit is measured on, and with a named defect (MUTANTS) in f32 it stands in for a wrong kernel in the host test.

Operand families (a Launch carries one):

* exact -- small integers or multiples of 1/4, so that any f32 evaluation order returns the f64 result; the output is compared BITWISE.
  LayerNorm on constant rows returns beta (beta2 under the second norm) -- the constant is picked per width so that fl(c D) fl(1 / D) = c, the host
  test holds the premise; the attention one-hot (one key scores 40, the rest 0, V integers 1 .. 255) returns the target's V row; the resampler on
  a unit impulse returns the tap table's own values; the VQ search on signed unit vectors scores 0 / -2 / -4 and the lowest index must win.
* uniform -- the result is a count or a mean of integers (attention with q = 0, the relative-key one-hot whose clamped distance row is shared by
  several keys, attnstats without or with constant logits, ctxpool / statspool on integer rows): within 2 ulp of the f64 quotient (variances
  within 4: they are compared as the square of the returned deviation).
* wide -- log-normal magnitudes of either sign, rows whose mean is 100 .. 1000 times their spread, softmax scores spanning +-8 (+-1e4 for the
  attnstats logits), pointwise arguments across each function's regimes (softplus threshold 20, erf tails at +-6, sigmoid at +-90); held to the
  limit below.
* index -- the VQ search on random unit codebooks: the f64 argmax wherever the f64 margin exceeds VQ_MARGIN; at most 1 % of the rows exempt.

The limit of the wide family is measured on the reference side, never on the kernels: E(op) is the largest elementwise error of the plain-f32
evaluation against f64 over all the op's wide launches, divided by the op's normaliser; the engine is held to 4 E with the same normaliser (the
margin of test_layernorm_vs_torch and attn_matrix.py: another accumulation order, not a worse one).  E is per op, not per case: a case whose f32
baseline happens to round exactly (one-element rows, a mean that is a power of two) would otherwise get a limit of 0.  The framed spectrum alone
takes E per case (E_of): its baseline is torch's own f32 FFT, a case is one FFT length and bank with hundreds of outputs, and a bank that lets a
dominant DC bin through (n1024-m100) would otherwise set the limit of every other configuration.

Normalisers -- the sum of magnitudes of what the op adds up, so they do not vanish where the result cancels:

  dot products, convs, pooling        sum |a| |b| (+ |bias|)
  softmax-weighted sums               sum_t w_t |v_t|
  LayerNorm, GroupNorm, colnorm       y = (x - mu) r g + b with r = 1 / sqrt(var + eps).  Any f32 evaluation holds mu as an f32 number: the sum
                                      behind it and its own rounding leave d_mu = O(A u), A = mean |x| >= |mu|, u = 2^-24 (A, not |mu|: the sum of
                                      a row that cancels still rounds at the size of its terms), and x - fl(mu) is exact where x is within a factor
                                      2 of mu (Sterbenz), so d_mu reaches every element unattenuated: |dy| <~ r |g| (u |x - mu| + d_mu) + u |b|.
                                      A shifted centre moves the variance by d_mu^2 only (second order).  Normaliser: r |g| (|x - mu| + A) + |b|;
                                      a second norm reads an input known to u n1 only, which moves its deviations by dd = n1_i + mean(n1) and its
                                      r2 by r2^3 mean(|d2| dd): r2 |g2| (dd + |d2| r2^2 mean(|d2| dd)) is added; through Mish (slope at most 1.09),
                                      1.09 times the normaliser plus |out|.
  statspool / attnstats deviation     the variance is compared, not its root (the root of a floored rounding residue is meaningless): out[C + c]^2
                                      against max(var, eps) with the normaliser var + u A^2 (A = the weighted mean of |x|): the centre's d_mu = O(A u)
                                      adds d_mu^2 to the variance, u A^2 in units of u.
  GELU, GEGLU, SiLU, Mish, gates      the product of the magnitudes of the factors (GELU: |0.5 v| (1 + |erf|)), plus 2^-102 |a|: a factor under the
                                      smallest normal f32 (sigmoid at -90) may be flushed to zero, 2^-126 in units of u.
  l2norm                              |out| (a product of three factors)
  fbank                               compared with take_log = 0, in the linear domain: R_t = the f64 rms over the bins of |X_f| for the frame;
                                      power 2: sum_f mel[m][f] (|X_f| + R_t) R_t, power 1: sum_f mel[m][f] R_t.  With take_log = 1 the same limit
                                      divided by max(ref_linear, floor), plus |log| for the f32 rounding of the logarithm's own value.

Canaries and poison: the GPU test pre-fills every output with a NaN bit pattern and a sentinel tail; a Launch's `valid` mask names the elements the
op must write, `ignore` the ones it may write with anything (the sequences whose neighbours hold NaN in the other pass of a conv case), everything
else must keep the pattern.  Inputs the op may not read hold NaN: x columns past C under ld_x > C, waveform past n_samples within the row stride,
K / V rows outside every key range, the neighbouring sequences of the sequence-bounded convs (two passes with the roles swapped).  Every index of
every table is in range.

Not in the matrix: the fused partial / bias flags of ln_kernel are not reachable through itts_layernorm_forward and stay with tests/test_gpu_gpt.py.
A second grid-stride pass needs more than 65536 * 8 * 256 elements (grid_for's cap); only ReLU runs at that size (BIG_RELU, generated and checked on
the device), the other pointwise kernels share the loop's form but are not run there.  VQ search with cd = 1 is all ties, so it is in the tie
family only.  The mutant "softplus without the threshold" is not listed: in f32 log1p(exp(v)) = v for every v > 20 up to the overflow of exp, and beyond it
v tanh(inf) = v as well, so no operand tells the two forms apart."""
import collections
import functools
import math
import zlib

import numpy as np
import torch

NAN = float("nan")
U = 2.0 ** -24
FLUSH = 2.0 ** -102
MARGIN = 4.0
VQ_MARGIN = 1e-5
VQ_EXEMPT_SHARE = 0.01
ATTN_REL_MAX = 512
LN_EPS = 1e-5

Case = collections.namedtuple("Case", "op name p")                      # p: a tuple of (key, value) pairs
Launch = collections.namedtuple("Launch", "label family args ref norm valid ignore")
# args: what the engine call needs (CPU tensors, scalars); ref / norm: f64, shaped like the framed output body; valid / ignore: bool masks of it


def P(c):
    return dict(c.p)


def case_id(c):
    return f"{c.op}-{c.name}"


def _case(op, name, **p):
    return Case(op, name, tuple(sorted(p.items())))


def _gen(c, salt):
    return torch.Generator().manual_seed((zlib.crc32(case_id(c).encode()) * 16 + salt) & 0x7FFFFFFFFFFF)


def _ints(gen, shape, lo, hi):
    """integers lo .. hi as f32 (never -0)"""
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _quarters(gen, shape, lim):
    return torch.randint(-4 * lim, 4 * lim + 1, shape, generator=gen).float() / 4


def _lognormal(gen, shape, sigma=1.5):
    return torch.randn(shape, generator=gen) * torch.exp(sigma * torch.randn(shape, generator=gen))


def _regimes(gen, n, hi, points):
    """n arguments of either sign with log-uniform magnitudes in [1e-6, hi], the named points and their f32 neighbours among them"""
    mag = torch.exp(torch.empty(n).uniform_(math.log(1e-6), math.log(hi), generator=gen))
    x = mag * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
    pts = torch.tensor([s * p for p in points for s in (1.0, -1.0)] + [0.0], dtype=torch.float32)
    nz = pts[pts != 0]                                                  # (0 has denormal neighbours: not an operand of these ops)
    pts = torch.cat([pts, torch.nextafter(nz, torch.full_like(nz, 1e9)), torch.nextafter(nz, torch.full_like(nz, -1e9))])
    m = min(n, pts.numel())
    x[torch.randperm(n, generator=gen)[:m]] = pts[:m]
    return x


def f32_ulp(x):
    _, e = torch.frexp(x.double().abs())
    return torch.where(x == 0, torch.zeros((), dtype=torch.float64), torch.ldexp(torch.ones((), dtype=torch.float64), e - 24))


def _tables(lens):
    """(tok_seq, tok_t, start, T) int32 of sequences packed back to back"""
    T = torch.tensor(list(lens), dtype=torch.int32)
    start = torch.cumsum(T, 0, dtype=torch.int32) - T
    tok_seq = torch.repeat_interleave(torch.arange(len(lens), dtype=torch.int32), T.long())
    tok_t = torch.arange(int(T.sum()), dtype=torch.int32) - start[tok_seq.long()]
    return tok_seq, tok_t, start, T


# =======================================================================================================================================
# the dispatch rules of the launchers, restated (gpt_kernels.hip: launch_ln; codec_kernels.hip: attention_launch)
# =======================================================================================================================================
LN_NV = (1, 2, 3, 4, 5, 6, 8)                                           # ln_kernel<NV>: D = 256 NV
LN_NE_ALL = (1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 20, 24, 32)           # ln_small_kernel<NE> as instantiated: D = 64 NE
LN_NE = tuple(ne for ne in LN_NE_ALL if ne % 4)                         # ... as reachable: a multiple of 256 goes to ln_kernel (7 widths)
LN_ROWS = (1, 3, 4, 5, 255, 256, 257)
LN_GENERIC_D = (1, 3, 36, 63, 65, 160, 1000)


def ln_instance(D, rows, second):
    """The kernel (and block shape) launch_ln picks, or None where itts_layernorm_forward refuses."""
    if D % 256 == 0:
        return f"ln_kernel<{D // 256}>/wpb{1 if rows <= 256 else 4}" if D // 256 in LN_NV else None
    if D % 64 == 0:
        return f"ln_small_kernel<{D // 64}>" if D // 64 in LN_NE else None
    return None if second else "ln_generic_kernel"


def attn_instance(dv, rel):
    return f"attn_generic_kernel<{16 if dv <= 64 else 32}>" + ("/relkey" if rel else "")


ONE_KERNEL = {"vq_project": "vq_project_kernel", "vq_search": "vq_search_kernel", "gather_conv": "gather_conv_kernel",
              "gelu": "gelu_erf_kernel", "scale_residual": "scale_residual_kernel", "groupnorm_mish": "groupnorm1_mish_kernel",
              "l2norm": "l2norm_kernel", "affine": "affine_act_kernel", "ctxpool": "ctxpool_kernel", "gate": "gate_kernel",
              "statspool": "statspool_kernel", "resample": "resample_kernel", "fbank": "fbank_kernel"}


def instances_of(c):
    """Every kernel instance (with the launcher branch, where it has one) the case's launches run on."""
    p = P(c)
    if c.op == "layernorm":
        return sorted({ln_instance(p["D"], r, s) for r in LN_ROWS for s in ((False, True) if p["D"] % 64 == 0 else (False,))})
    if c.op == "attention":
        return [attn_instance(p["dv"], p["rel"] is not None)]
    if c.op == "dwconv":
        return ["dwconv_kernel/causal" if p["causal"] else "dwconv_kernel/same"]
    if c.op == "glu":
        return [f"glu_kernel/mode{p['mode']}"]
    if c.op == "act":
        return [f"act_kernel/mode{p['mode']}"]
    if c.op == "attnstats":
        return ["attnstats_kernel/" + p["logits"]]
    if c.op == "colnorm":
        return [f"colnorm_kernel/mode{p['mode']}"]
    return [ONE_KERNEL[c.op]]


ALL_INSTANCES = ([f"ln_kernel<{nv}>/wpb{w}" for nv in LN_NV for w in (1, 4)] + [f"ln_small_kernel<{ne}>" for ne in LN_NE] + ["ln_generic_kernel"] +
                 [f"attn_generic_kernel<{d}>{r}" for d in (16, 32) for r in ("", "/relkey")] + ["dwconv_kernel/same", "dwconv_kernel/causal"] +
                 ["glu_kernel/mode0", "glu_kernel/mode1", "act_kernel/mode0", "act_kernel/mode1", "act_kernel/mode2"] +
                 ["attnstats_kernel/none", "attnstats_kernel/const", "attnstats_kernel/onehot", "attnstats_kernel/wide"] +
                 ["colnorm_kernel/mode0", "colnorm_kernel/mode1"] + sorted(ONE_KERNEL.values()))


# =======================================================================================================================================
# LayerNorm
# =======================================================================================================================================
def ln_constant(D):
    """A row constant c with fl(fl(c D) fl(1 / D)) == c in f32: the kernels' mean of a constant row is then c, every deviation 0."""
    invD = np.float32(1.0) / np.float32(D)
    for c in (3.0, 5.0, 2.0, -7.0, 6.0, -1.5, 1.0, 10.0, 12.0, 0.75):
        if np.float32(np.float32(c) * np.float32(D)) * invD == np.float32(c):
            return c
    raise AssertionError(f"no exact constant for D = {D}")


def ln_eval(a, dt, mutant=None):
    eps, D = a["eps"], a["x"].shape[1]

    def one(v, g, b, nin=None):
        mu = v.mean(-1, keepdim=True)
        d = v - mu
        if mutant == "ln:one_pass_variance":
            var = (v * v).mean(-1, keepdim=True) - mu * mu
        elif mutant == "ln:unbiased_variance":
            var = (d * d).sum(-1, keepdim=True) / max(D - 1, 1)
        else:
            var = (d * d).mean(-1, keepdim=True)
        r = 1 / (var.clamp(min=0).sqrt() + eps) if mutant == "ln:eps_outside_root" else 1 / (var + eps).sqrt()
        n = r * g.abs() * (d.abs() + v.abs().mean(-1, keepdim=True)) + b.abs()
        if nin is not None:
            # an input known to u nin: the deviation moves by nin_i + mean(nin) (its own error and the mean's), r by r^3 mean(|d| that)
            dd = nin + nin.mean(-1, keepdim=True)
            n = n + r * g.abs() * (dd + d.abs() * r * r * (d.abs() * dd).mean(-1, keepdim=True))
        return d * r * g + b, n
    y, n = one(a["x"].to(dt), a["g"].to(dt), a["b"].to(dt))
    if a.get("g2") is not None:
        y, n = one(y, a["g2"].to(dt), a["b2"].to(dt), n)
    return y, n


def ln_cases():
    Ds = [256 * nv for nv in LN_NV] + [64 * ne for ne in LN_NE] + list(LN_GENERIC_D)
    return [_case("layernorm", f"D{D}", D=D) for D in Ds]


def ln_launches(c, families=("exact", "wide")):
    D = P(c)["D"]
    for rows in LN_ROWS:
        for second in ((False, True) if D % 64 == 0 else (False,)):
            gen = _gen(c, rows * 2 + second)
            g, b, g2, b2 = (torch.randn(D, generator=gen) for _ in range(4))
            tag = f"rows{rows}" + ("-second" if second else "")
            valid = torch.ones(rows, D, dtype=torch.bool)
            if "exact" in families:
                cst = ln_constant(D)
                a = dict(x=torch.full((rows, D), cst), g=g, b=torch.full((D,), cst) if second else b, g2=g2 if second else None,
                         b2=b2 if second else None, eps=LN_EPS)
                want = (b2 if second else b).double()[None, :].expand(rows, D).clone()
                yield Launch("exact-" + tag, "exact", a, want, None, valid, None)
            if "wide" in families:
                kind = torch.arange(rows)[:, None] % 3
                spread = torch.exp(torch.randn(rows, 1, generator=gen))
                off = spread * torch.empty(rows, 1).uniform_(100, 1000, generator=gen) * (torch.randint(0, 2, (rows, 1), generator=gen) * 2 - 1)
                x = torch.where(kind == 0, off + spread * torch.randn(rows, D, generator=gen),
                                torch.where(kind == 1, 0.01 * torch.randn(rows, D, generator=gen), _lognormal(gen, (rows, D))))
                a = dict(x=x, g=g, b=b, g2=g2 if second else None, b2=b2 if second else None, eps=LN_EPS)
                ref, norm = ln_eval(a, torch.float64)
                yield Launch("wide-" + tag, "wide", a, ref, norm, valid, None)


LN_REFUSALS = ((448, False), (1792, False), (36, True), (1000, True))      # (D, second): launch_ln returns before any launch


# =======================================================================================================================================
# the generic packed attention, with and without the relative-key bias
# =======================================================================================================================================
ATTN_KLENS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
ATTN_TARGETS = ("0", "1", "62", "63", "64", "65", "klen-2", "klen-1")
Q_HOT, K_HOT, EXACT_SCALE = 16.0, 20.0, 0.125                          # 16 * 20 / 8 = 40


def attn_cases():
    cs = []
    for dq, dv, H in ((4, 4, 1), (24, 20, 3), (64, 64, 3), (128, 68, 1), (256, 128, 3), (64, 128, 1)):
        cs.append(_case("attention", f"dq{dq}-dv{dv}-h{H}", dq=dq, dv=dv, H=H, rel=None))
    for (left, right), (dq, dv, H) in zip(((0, 0), (9, 4), (64, 8), (255, 256)), ((24, 20, 3), (64, 64, 1), (64, 68, 3), (128, 128, 1))):
        cs.append(_case("attention", f"rel{left}-{right}-dq{dq}-dv{dv}-h{H}", dq=dq, dv=dv, H=H, rel=(left, right)))
    return cs


def attn_geometry(c):
    """Key sequences of every length of ATTN_KLENS (600 more under the relative key, to pass both clamps of the widest table) laid out with gaps
    (kstart nonzero), and the queries of different sequences interleaved.  -> (kstart, klen, qpos, n_keys, used rows mask)"""
    rel = P(c)["rel"] is not None
    lens = list(ATTN_KLENS) + ([600] if rel else [])
    starts, pos = [], 3
    for n in lens:
        starts.append(pos)
        pos += n + 2                                                   # two rows no query may read between the sequences
    nk = pos + 1
    per = 5 if rel else 2
    qs = [(s, i) for i in range(per) for s in range(len(lens))]        # interleaved: consecutive queries belong to different sequences
    kstart = torch.tensor([starts[s] for s, _ in qs], dtype=torch.int32)
    klen = torch.tensor([lens[s] for s, _ in qs], dtype=torch.int32)
    # relative key: the query's position in its range -- both ends (the whole range on one side), the middle, one off each end
    qpos = torch.tensor([min(max(0, (0, lens[s] - 1, lens[s] // 2, 1, lens[s] - 2)[i] if rel else 0), max(lens[s] - 1, 0)) for s, i in qs],
                        dtype=torch.int32)
    used = torch.zeros(nk, dtype=torch.bool)
    for s, n in zip(starts, lens):
        used[s:s + n] = True
    return kstart, klen, qpos, nk, used


def attn_eval(a, dt, mutant=None):
    q, k, v = a["q"].to(dt), a["k"].to(dt), a["v"].to(dt)
    nq, H, dq = q.shape
    nk = k.shape[0]
    ks, kl = a["kstart"].long(), a["klen"].long()
    used = a["used"]
    k = torch.where(used[:, None, None], k, torch.zeros((), dtype=dt))
    v = torch.where(used[:, None, None], v, torch.zeros((), dtype=dt))
    j = torch.arange(nk)[None, :] - ks[:, None]                        # the key's index inside the query's range
    lo, hi = torch.zeros_like(kl), kl - 1
    if mutant == "attn:first-1":
        lo = lo - 1
    elif mutant == "attn:first+1":
        lo = lo + 1
    elif mutant == "attn:last+1":
        hi = hi + 1
    elif mutant == "attn:last-1":
        hi = hi - 1
    mask = (j >= lo[:, None]) & (j <= hi[:, None]) & (torch.arange(nk)[None, :] >= 0)
    if mutant in ("attn:drop@63", "attn:drop@64"):
        mask = mask & (j != int(mutant[-2:]))
    elif mutant == "attn:drop@last":
        mask = mask & (j != (kl - 1)[:, None])
    s = torch.einsum("mhd,khd->mhk", q, k)
    if a.get("emb") is not None:
        left, right = a["left"], a["right"]
        dist = j - a["qpos"].long()[:, None]
        if mutant == "rel:sign":
            dist = -dist
        cl, cr = -left, right
        if mutant == "rel:left_clamp":
            cl = min(cl + 1, cr)
        elif mutant == "rel:right_clamp":
            cr = max(cr - 1, cl)
        qe = torch.einsum("mhd,rd->mhr", q, a["emb"].to(dt))           # [nq][H][left + right + 1]
        if mutant == "rel:no_clamp":
            r = dist + left
            inside = (r >= 0) & (r <= left + right)
            bias = torch.gather(qe, 2, r.clamp(0, left + right)[:, None, :].expand(nq, H, nk)) * inside[:, None, :]
        else:
            bias = torch.gather(qe, 2, (dist.clamp(cl, cr) + left)[:, None, :].expand(nq, H, nk))
        s = s + bias
    s = s * a["scale"]
    m = mask[:, None, :]
    w = torch.softmax(torch.where(m, s, torch.full((), -math.inf, dtype=dt)), dim=-1)
    w = torch.where(m.any(-1, keepdim=True), w, torch.zeros((), dtype=dt))        # klen 0: zeros, as the reference's masked softmax
    return torch.einsum("mhk,khe->mhe", w, v), torch.einsum("mhk,khe->mhe", w, v.abs())


def _attn_poisoned(x, used):
    return torch.where(used[:, None, None], x, torch.full((), NAN))


def attn_launches(c, families=("exact", "uniform", "wide")):
    p = P(c)
    dq, dv, H, rel = p["dq"], p["dv"], p["H"], p["rel"]
    kstart, klen, qpos, nk, used = attn_geometry(c)
    nq = kstart.numel()
    gen = _gen(c, 1)
    base = dict(kstart=kstart, klen=klen, used=used, H=H, dq=dq, dv=dv)
    valid = torch.ones(nq, H, dv, dtype=torch.bool)
    # V integers 1 .. 255; of either sign without the relative key (with it the shared-weight mean must not cancel: the leftover weights would show)
    sign = torch.randint(0, 2, (nk, H, dv), generator=gen).float() * 2 - 1
    vint = _attn_poisoned(_ints(gen, (nk, H, dv), 1, 255) * (sign if rel is None else 1.0), used)
    if rel is not None:
        left, right = rel
        base.update(qpos=qpos, left=left, right=right)
    if "exact" in families and rel is None:
        for rule in ATTN_TARGETS:
            tgt = torch.tensor([(int(rule) if rule.isdigit() else n + int(rule[4:])) for n in klen.tolist()])
            tgt = torch.where((tgt >= 0) & (tgt < klen), tgt, torch.zeros_like(tgt))              # where the range lacks the key: key 0
            if rule != "0" and not bool((tgt > 0).any()):
                continue
            q = torch.zeros(nq, H, dq)
            k = _attn_poisoned(torch.zeros(nk, H, dq), used)
            want = torch.zeros(nq, H, dv, dtype=torch.float64)
            for m in range(nq):
                if int(klen[m]) == 0:
                    continue
                row = int(kstart[m]) + int(tgt[m])                     # (the queries of one sequence share the target under a rule)
                for h in range(H):
                    q[m, h, (m + h) % dq] = Q_HOT
                    k[row, h, (m + h) % dq] = K_HOT
                    want[m, h] = vint[row, h].double()
            yield Launch("onehot@" + rule, "exact", dict(base, q=q, k=k, v=vint, scale=EXACT_SCALE), want, None, valid, None)
    if "uniform" in families:
        k = _attn_poisoned(_ints(gen, (nk, H, dq), -3, 3), used)
        if rel is None:
            a = dict(base, q=torch.zeros(nq, H, dq), k=k, v=vint, scale=EXACT_SCALE)
            yield Launch("uniform", "uniform", a, attn_eval(a, torch.float64)[0], None, valid, None)
        else:
            # q . K = 0 (K is 0 in the query's dimension); one row r of the distance table scores 40: the keys at clamped distance r share the weight
            rows = sorted({0, left + right, left, max(left - 1, 0), min(left + 1, left + right), (left + right) // 2})
            for r in rows:
                q = torch.zeros(nq, H, dq)
                q[:, :, 1] = Q_HOT
                k2 = k.clone()
                k2[:, :, 1] = torch.where(used[:, None], torch.zeros(()), torch.full((), NAN))
                emb = _ints(gen, (left + right + 1, dq), -3, 3)
                emb[:, 1] = 0
                emb[r, 1] = K_HOT
                a = dict(base, q=q, k=k2, v=vint, emb=emb, scale=EXACT_SCALE)
                yield Launch(f"relhot@{r}", "uniform", a, attn_eval(a, torch.float64)[0], None, valid, None)
    if "wide" in families:
        q = torch.randn(nq, H, dq, generator=gen) * 2.5                # q . k / sqrt(dq) has a standard deviation of 2.5: about +-8 over 200 keys
        k = _attn_poisoned(torch.randn(nk, H, dq, generator=gen), used)
        v = _attn_poisoned(_lognormal(gen, (nk, H, dv)), used)
        a = dict(base, q=q, k=k, v=v, scale=1.0 / math.sqrt(dq))
        if rel is not None:
            a["emb"] = torch.randn(left + right + 1, dq, generator=gen) * 0.5
        ref, norm = attn_eval(a, torch.float64)
        yield Launch("wide", "wide", a, ref, norm, valid, None)


def onehot_leftover(c):
    """The largest total weight of the keys beside the target, times the largest |V|, over the case's queries: must stay under half an ulp of the
    smallest |V| = 1 (2^-25, the step below 1) for the one-hot output to be the V row bitwise."""
    return (int(max(ATTN_KLENS)) - 1) * math.exp(-40.0) * 255.0


ATTN_REFUSALS = (dict(dq=64, dv=132), dict(dq=6, dv=64), dict(dq=64, dv=64, left=256, right=256))


# =======================================================================================================================================
# pointwise ops: gelu, glu / geglu, relu / silu / tanh, sigmoid gate, scale_residual, affine
# =======================================================================================================================================
POINT_SIZES = ((1, 1), (85, 3), (256, 1), (1, 257), (5, 257), (301, 3))      # (n, C): n C = 1, 255, 256, 257, 1285, 903; C odd


def _erf(x):
    return torch.erf(x)


def _sigmoid(x):
    return 1 / (1 + torch.exp(-x))


def point_eval(a, dt, mutant=None):
    op, mode = a["op"], a.get("mode", 0)
    x = a["x"].to(dt)
    if op == "gelu" or (op == "glu" and mode == 1):
        v = x if op == "gelu" else x[:, a["C"]:]
        if mutant == "gelu:tanh_form":
            gl = 0.5 * v * (1 + torch.tanh(math.sqrt(2 / math.pi) * (v + 0.044715 * v ** 3)))
        else:
            gl = 0.5 * v * (1 + _erf(v * math.sqrt(0.5)))
        gn = (0.5 * v).abs() * (1 + _erf(v * math.sqrt(0.5)).abs())
        if op == "gelu":
            return gl, gn + FLUSH
        first = x[:, :a["C"]]
        return first * gl, first.abs() * gn + FLUSH * first.abs()
    if op == "glu":
        first, b = x[:, :a["C"]], x[:, a["C"]:]
        return first * _sigmoid(b), first.abs() * (_sigmoid(b) + FLUSH)
    if op == "act":
        if mode == 0:
            return x.clamp(min=0), None
        if mode == 1:
            return x * _sigmoid(x), x.abs() * (_sigmoid(x) + FLUSH)
        return torch.tanh(x), torch.tanh(x).abs() + FLUSH
    if op == "gate":
        g = a["g"].to(dt)
        return x * _sigmoid(g), x.abs() * (_sigmoid(g) + FLUSH)
    if op == "scale_residual":
        y, gam = a["y"].to(dt), a["gamma"].to(dt)
        return x + gam * y, x.abs() + (gam * y).abs()
    if op == "affine":
        xs = x[:, :a["C"]]
        v = xs * a["scale"].to(dt) + a["shift"].to(dt)
        return (v.clamp(min=0) if a["relu"] else v), (xs * a["scale"].to(dt)).abs() + a["shift"].to(dt).abs()
    raise KeyError(op)


def point_cases():
    cs = [_case("gelu", "all"), _case("gate", "all"), _case("scale_residual", "all"), _case("affine", "all")]
    cs += [_case("glu", f"mode{m}", mode=m) for m in (0, 1)] + [_case("act", f"mode{m}", mode=m) for m in (0, 1, 2)]
    return cs


def point_launches(c, families=("exact", "wide")):
    op, mode = c.op, P(c).get("mode", 0)
    for n, C in POINT_SIZES:
        gen = _gen(c, n * 1000 + C)
        tag = f"n{n}-C{C}"
        valid = torch.ones(n, C, dtype=torch.bool)
        if op in ("gelu", "gate") or (op == "act" and mode):
            if "wide" not in families:
                continue
            hi, pts = {"gelu": (12.0, (6.0, 4.0, 1.0)), "gate": (95.0, (90.0, 87.0, 20.0)), "act": ((95.0, (90.0, 87.0)) if mode == 1 else (12.0, (9.0, 1.0)))}[op]
            a = dict(op=op, mode=mode, x=_regimes(gen, n * C, hi, pts).view(n, C), C=C)
            if op == "gate":
                a["g"] = a["x"]
                a["x"] = _lognormal(gen, (n, C))
            ref, norm = point_eval(a, torch.float64)
            yield Launch("wide-" + tag, "wide", a, ref, norm, valid, None)
        elif op == "act":
            if "exact" in families:
                a = dict(op=op, mode=0, x=_lognormal(gen, (n, C)), C=C)
                yield Launch("exact-" + tag, "exact", a, point_eval(a, torch.float64)[0], None, valid, None)
        elif op == "glu":
            if "wide" not in families:
                continue
            hi, pts = ((95.0, (90.0, 87.0, 20.0)) if mode == 0 else (12.0, (6.0, 4.0, 1.0)))
            x = torch.cat([_lognormal(gen, (n, C)), _regimes(gen, n * C, hi, pts).view(n, C)], 1)
            a = dict(op=op, mode=mode, x=x, C=C)
            ref, norm = point_eval(a, torch.float64)
            yield Launch("wide-" + tag, "wide", a, ref, norm, valid, None)
        elif op == "scale_residual":
            for fam in families:
                if fam == "exact":
                    a = dict(op=op, x=_quarters(gen, (n, C), 8), y=_ints(gen, (n, C), -8, 8), gamma=_quarters(gen, (C,), 2), C=C)
                elif fam == "wide":
                    a = dict(op=op, x=_lognormal(gen, (n, C)), y=_lognormal(gen, (n, C)), gamma=torch.randn(C, generator=gen), C=C)
                else:
                    continue
                ref, norm = point_eval(a, torch.float64)
                yield Launch(f"{fam}-{tag}", fam, a, ref, norm if fam == "wide" else None, valid, None)
        elif op == "affine":
            for fam in families:
                for relu in (0, 1):
                    for ld in (C, C + 3):
                        if fam == "exact":
                            x, sc, sh = _quarters(gen, (n, ld), 8), _quarters(gen, (C,), 2), _quarters(gen, (C,), 8)
                        elif fam == "wide":
                            x, sc, sh = _lognormal(gen, (n, ld)), torch.randn(C, generator=gen), _lognormal(gen, (C,))
                        else:
                            continue
                        x[:, C:] = NAN                                  # columns past C under ld_x > C: never read
                        a = dict(op=op, x=x, scale=sc, shift=sh, relu=relu, C=C, ld=ld)
                        ref, norm = point_eval(a, torch.float64)
                        yield Launch(f"{fam}-{tag}-ld{ld}-relu{relu}", fam, a, ref, norm if fam == "wide" else None, valid, None)


BIG_RELU = 65536 * 8 * 256 + 257        # one element count past a single grid-stride pass of the largest grid grid_for() returns (the GPU test only)


# =======================================================================================================================================
# sequence-bounded depthwise convs (same-padded and causal), gather-conv im2col with nearest interpolation
# =======================================================================================================================================
def dwconv_cases():
    cs = []
    for causal, ks in ((0, (1, 3, 7, 31)), (1, (1, 2, 7, 31))):
        for k, C in zip(ks, (1, 48, 257, 48)):
            cs.append(_case("dwconv", f"{'causal' if causal else 'same'}-k{k}-C{C}", causal=causal, k=k, C=C))
    return cs


def dwconv_eval(a, dt, mutant=None):
    x, w = a["x"].to(dt), a["w"].to(dt)
    k, n, C = a["k"], x.shape[0], x.shape[1]
    causal = a["causal"] ^ (mutant == "dwconv:padding")
    padl = k - 1 if causal else (k - 1) // 2
    t, T = a["tok_t"].long(), a["seq_T"].long()[a["tok_seq"].long()]
    out = a["b"].to(dt)[None, :].expand(n, C).clone() if a["b"] is not None else torch.zeros(n, C, dtype=dt)
    norm = out.abs()
    m = torch.arange(n)
    for j in range(k):
        u = t + j - padl
        ok = (u >= 0) & (u < T)
        src = torch.where(ok, m + j - padl, m)
        term = torch.where(ok[:, None], x[src] * w[:, j][None, :], torch.zeros((), dtype=dt))
        out, norm = out + term, norm + term.abs()
    return out, norm


def dwconv_launches(c, families=("exact", "wide")):
    p = P(c)
    k, C, causal = p["k"], p["C"], p["causal"]
    lens = [0, 1, 2, max(k - 1, 1), k, k + 1, 0, 40, 3, 2 * k + 1]
    tok_seq, tok_t, _, T = _tables(lens)
    n = int(T.sum())
    for fam in families:
        if fam not in ("exact", "wide"):
            continue
        gen = _gen(c, 1 + (fam == "wide"))
        if fam == "exact":
            x, w, b = _ints(gen, (n, C), -8, 8), _quarters(gen, (C, k), 2), _quarters(gen, (C,), 8)
        else:
            x, w, b = _lognormal(gen, (n, C)), torch.randn(C, k, generator=gen), _lognormal(gen, (C,))
        for parity in (0, 1):
            # the sequences of the other parity hold NaN: a tap that leaves its sequence returns NaN; their own outputs may be anything
            mine = (tok_seq % 2 == parity)
            xp = torch.where(mine[:, None], x, torch.full((), NAN))
            a = dict(x=xp, w=w, b=None if (causal and parity) else b, tok_seq=tok_seq, tok_t=tok_t, seq_T=T, k=k, causal=causal)
            ref, norm = dwconv_eval(dict(a, x=x), torch.float64)
            valid = mine[:, None].expand(n, C).clone()
            yield Launch(f"{fam}-pass{parity}", fam, a, ref, norm if fam == "wide" else None, valid, ~valid)


GATHER_PAIRS = ((1, 1), (1, 7), (9, 15), (9, 18), (30, 60), (700, 1204), (7, 3))


def nearest_index(u, Ts, Td, exact=False):
    """torch's nearest rule: f32 scale Ts / Td, floorf(u scale), min(., Ts - 1); exact: the rational floor"""
    u = np.asarray(u)
    if Ts == Td:
        return u.astype(np.int64)
    if exact:
        return np.minimum((u.astype(np.int64) * Ts) // Td, Ts - 1)
    scale = np.float32(Ts) / np.float32(Td)
    return np.minimum(np.floor(u.astype(np.float32) * scale).astype(np.int64), Ts - 1)


@functools.lru_cache(maxsize=1)
def floor_disagreeing_pairs(limit=3):
    """(Ts, Td) whose f32 floor differs from the exact rational floor somewhere (found on the CPU, smallest first)"""
    found = []
    for Td in range(2, 200):
        for Ts in range(2, 200):
            if Ts != Td:
                u = np.arange(Td)
                if (nearest_index(u, Ts, Td) != nearest_index(u, Ts, Td, True)).any():
                    found.append((Ts, Td))
                    if len(found) == limit:
                        return tuple(found)
    return tuple(found)


def gather_cases():
    return [_case("gather_conv", f"k{k}-C{C}", k=k, C=C) for k, C in ((1, 4), (3, 64), (5, 4), (3, 4))]


def gather_eval(a, dt, mutant=None):
    x = a["x"].to(dt)
    k, C = a["k"], x.shape[1]
    n = a["tok_seq"].numel()
    col = torch.zeros(n, k, C, dtype=dt)
    seq, t = a["tok_seq"].long(), a["tok_t"].long()
    for s in range(a["src_T"].numel()):
        Ts, Td, st = int(a["src_T"][s]), int(a["dst_T"][s]), int(a["src_start"][s])
        rows = (seq == s).nonzero().flatten()
        for j in range(k):
            u = t[rows] + j - (k - 1) // 2
            ok = (u >= 0) & (u < Td)
            si = torch.from_numpy(nearest_index(u.clamp(0, max(Td - 1, 0)).numpy(), Ts, Td, exact=(mutant == "gather:exact_floor")))
            col[rows, j] = torch.where(ok[:, None], x[st + si], torch.zeros((), dtype=dt))
    return col.view(n, k * C), None


def gather_launches(c, families=("exact",)):
    if "exact" not in families:
        return
    p = P(c)
    k, C = p["k"], p["C"]
    pairs = list(GATHER_PAIRS) + list(floor_disagreeing_pairs())
    gen = _gen(c, 1)
    src_T = torch.tensor([a for a, _ in pairs], dtype=torch.int32)
    dst_T = torch.tensor([b for _, b in pairs], dtype=torch.int32)
    src_start = torch.cumsum(src_T + 1, 0, dtype=torch.int32) - src_T          # one NaN row in front of and between the source sequences
    n_src = int(src_start[-1] + src_T[-1]) + 1
    x = torch.full((n_src, C), NAN)
    for s in range(len(pairs)):
        x[int(src_start[s]):int(src_start[s] + src_T[s])] = _lognormal(gen, (int(src_T[s]), C))
    tok_seq, tok_t, _, _ = _tables(dst_T.tolist())
    a = dict(x=x, tok_seq=tok_seq, tok_t=tok_t, src_start=src_start, src_T=src_T, dst_T=dst_T, k=k, C=C)
    ref, _ = gather_eval(a, torch.float64)
    yield Launch("copy", "exact", a, ref, None, torch.ones(tok_seq.numel(), k * C, dtype=torch.bool), None)


# =======================================================================================================================================
# GroupNorm(1) + Mish, l2norm, column normalisation
# =======================================================================================================================================
GN_LENS = (0, 1, 2, 15, 16, 17, 1025)


def gn_cases():
    return [_case("groupnorm_mish", f"C{C}", C=C) for C in (4, 64, 80)]


def gn_eval(a, dt, mutant=None):
    x = a["x"].to(dt)
    g, b = a["gamma"].to(dt), a["beta"].to(dt)
    out, norm = torch.full(x.shape, NAN, dtype=dt), torch.full(x.shape, NAN, dtype=dt)
    for s, T in zip(a["seq_start"].tolist(), a["seq_T"].tolist()):
        if T == 0:
            continue
        xs = x[s:s + T]
        mu = xs.mean()
        d = xs - mu
        var = (d * d).sum() / (max(xs.numel() - 1, 1) if mutant == "gn:unbiased_variance" else xs.numel())
        r = 1 / (var.sqrt() + a["eps"]) if mutant == "gn:eps_outside_root" else 1 / (var + a["eps"]).sqrt()
        v = d * r * g + b
        sp = torch.where(v > 20, v, torch.log1p(torch.exp(v.clamp(max=20))))
        out[s:s + T] = v * torch.tanh(sp)
        norm[s:s + T] = 1.09 * (r * g.abs() * (d.abs() + xs.abs().mean()) + b.abs()) + out[s:s + T].abs()
    return out, norm


def gn_launches(c, families=("wide",)):
    if "wide" not in families:
        return
    C = P(c)["C"]
    gen = _gen(c, 1)
    lens = list(GN_LENS) + [3]
    starts, pos = [], 1
    for T in lens:
        starts.append(pos)
        pos += T + 2                                                    # seq_start leaves gaps: rows that belong to no sequence
    n = pos
    valid = torch.zeros(n, C, dtype=torch.bool)
    x = torch.full((n, C), NAN)
    for i, (s, T) in enumerate(zip(starts, lens)):
        valid[s:s + T] = True
        body = _lognormal(gen, (T, C), 1.0)
        if i % 2:
            sp = float(torch.exp(torch.randn((), generator=gen)))
            body = sp * (300.0 * (1 if i % 4 == 1 else -1) + torch.randn(T, C, generator=gen))           # a mean of 300 spreads
        x[s:s + T] = body
    # gamma, beta reach past the softplus threshold: v spans about +-40
    a = dict(x=x, gamma=torch.randn(C, generator=gen) * 6, beta=torch.randn(C, generator=gen) * 8, seq_start=torch.tensor(starts, dtype=torch.int32),
             seq_T=torch.tensor(lens, dtype=torch.int32), eps=1e-5, C=C)
    ref, norm = gn_eval(a, torch.float64)
    yield Launch("wide", "wide", a, ref, norm, valid, None)


L2_C = (1, 63, 64, 65, 1280)


def l2_cases():
    return [_case("l2norm", f"C{C}", C=C) for C in L2_C]


def l2_eval(a, dt, mutant=None):
    x, g = a["x"].to(dt), a["gamma"].to(dt)
    nrm = (x * x).sum(-1, keepdim=True).sqrt().clamp(min=1e-12)
    out = x / nrm * a["scale"] * g
    return out, out.abs() + FLUSH


def l2_launches(c, families=("wide",)):
    if "wide" not in families:
        return
    C = P(c)["C"]
    gen = _gen(c, 1)
    x = _lognormal(gen, (7, C))
    x[3] = 0                                                           # a zero row gives 0, not NaN
    x[5] = x[5] * 1e-3
    a = dict(x=x, gamma=torch.randn(C, generator=gen), scale=math.sqrt(C))
    ref, norm = l2_eval(a, torch.float64)
    yield Launch("wide", "wide", a, ref, norm, torch.ones(7, C, dtype=torch.bool), None)


COLNORM_N = (1, 2, 255, 256, 257, 1000)


def colnorm_cases():
    return [_case("colnorm", f"mode{m}-n{n}", mode=m, n=n) for m in (0, 1) for n in COLNORM_N if not (m == 1 and n == 1)]


def colnorm_eval(a, dt, mutant=None):
    x = a["x"].to(dt)
    n = x.shape[0]
    mu = x.mean(0, keepdim=True)
    d = x - mu
    if a["mode"] == 0:
        return d, d.abs() + x.abs().mean(0, keepdim=True)
    ddof = a["ddof"] if mutant != "colnorm:ddof_swapped" else 1 - a["ddof"]
    var = (d * d).sum(0, keepdim=True) / max(n - ddof, 1)
    r = 1 / (var.sqrt() + a["eps"]) if mutant == "colnorm:eps_outside_root" else 1 / (var + a["eps"]).sqrt()
    return d * r, r * (d.abs() + x.abs().mean(0, keepdim=True))


def colnorm_launches(c, families=("wide",)):
    if "wide" not in families:
        return
    p = P(c)
    n, mode, C = p["n"], p["mode"], 5
    for ddof in ((0,) if mode == 0 else ((0, 1) if n > 1 else (0,))):
        gen = _gen(c, ddof)
        spread = torch.exp(torch.randn(1, C, generator=gen))
        spread[0, 1] = 0.003                                            # a column whose variance is comparable to eps
        mean = spread * torch.tensor([0.0, 0.0, 100.0, -1000.0, 300.0])[None, :]
        x = mean + spread * torch.randn(n, C, generator=gen)
        a = dict(x=x, mode=mode, ddof=ddof, eps=1e-7 if mode else 0.0, ld_out=C + 3)
        ref, norm = colnorm_eval(a, torch.float64)
        pad = torch.full((n, 3), NAN, dtype=torch.float64)
        valid = torch.cat([torch.ones(n, C, dtype=torch.bool), torch.zeros(n, 3, dtype=torch.bool)], 1)     # columns past C under ld_out > C keep the canary
        yield Launch(f"wide-ddof{ddof}", "wide", a, torch.cat([ref, pad], 1), torch.cat([norm, pad], 1), valid, None)


# =======================================================================================================================================
# pooling: context pooling, statistics pooling, attentive statistics pooling
# =======================================================================================================================================
POOL_N = (2, 3, 63, 64, 65, 300)
CTX_N = (1, 63, 64, 65, 99, 100, 101, 200, 250)


def ctx_cases():
    return [_case("ctxpool", f"n{n}", n=n) for n in CTX_N]


def ctx_eval(a, dt, mutant=None):
    h = a["x"].to(dt)
    n, seg = h.shape[0], a["seg_len"]
    out, norm = torch.empty_like(h), torch.empty_like(h)
    tot, atot = h.sum(0) / n, h.abs().sum(0) / n
    for s0 in range(0, n, seg):
        s1 = min(s0 + seg, n)
        div = seg if mutant == "ctxpool:last_segment_by_seg_len" else s1 - s0
        out[s0:s1] = tot + h[s0:s1].sum(0) / div
        norm[s0:s1] = atot + h[s0:s1].abs().sum(0) / (s1 - s0)
    return out, norm


def ctx_launches(c, families=("uniform", "wide")):
    n = P(c)["n"]
    for seg in sorted({1, 100, n, n + 1}):
        for C in (1, 5):
            gen = _gen(c, seg * 8 + C)
            for fam in families:
                if fam == "uniform":
                    x = _ints(gen, (n, C), 1, 255)                      # two quotients of one sign: their sum does not cancel
                elif fam == "wide":
                    x = _lognormal(gen, (n, C)) + torch.tensor([0.0, 50.0, -200.0, 0.0, 1.0])[:C]
                else:
                    continue
                a = dict(x=x, seg_len=seg)
                ref, norm = ctx_eval(a, torch.float64)
                yield Launch(f"{fam}-seg{seg}-C{C}", fam, a, ref, norm if fam == "wide" else None, torch.ones(n, C, dtype=torch.bool), None)


def stats_cases():
    cs = [_case("statspool", f"n{n}", n=n) for n in POOL_N]
    return cs + [_case("attnstats", f"{lg}-n{n}", n=n, logits=lg) for lg in ("none", "const", "onehot", "wide") for n in (1,) + POOL_N]


def stats_eval(a, dt, mutant=None):
    """-> ([2][C]: mean | VARIANCE (floored at eps for attnstats), normalisers)"""
    x = a["x"].to(dt)
    n = x.shape[0]
    if a["op"] == "statspool":
        mu = x.mean(0)
        d = x - mu
        var = (d * d).sum(0) / (n if mutant == "statspool:biased_variance" else n - 1)
        return torch.stack([mu, var]), torch.stack([x.abs().mean(0), var + U * x.abs().mean(0) ** 2 + FLUSH])
    if a["logit"] is None:
        w = torch.full_like(x, 1.0 / n)
    else:
        w = torch.softmax(a["logit"].to(dt), 0)
    mu = (w * x).sum(0)
    d = x - mu
    var = (w * d * d).sum(0)
    if mutant == "attnstats:unbiased_variance":
        var = var * n / max(n - 1, 1)
    var = var.clamp(min=a["eps"])
    return torch.stack([mu, var]), torch.stack([(w * x.abs()).sum(0), var + U * (w * x.abs()).sum(0) ** 2])


def stats_launches(c, families=("exact", "uniform", "wide")):
    p = P(c)
    n, C = p["n"], 5
    lg = p.get("logits")
    valid = torch.ones(2, C, dtype=torch.bool)
    for fam in families:
        gen = _gen(c, {"exact": 1, "uniform": 2, "wide": 3}.get(fam, 4))
        if fam == "uniform" and lg in (None, "none", "const"):
            x = _ints(gen, (n, C), -255, 255)
        elif fam == "wide" and lg != "onehot":
            spread = torch.exp(torch.randn(1, C, generator=gen))
            x = spread * (torch.tensor([0.0, 100.0, -1000.0, 300.0, 0.0])[None, :] + torch.randn(n, C, generator=gen))
        elif fam == "exact" and lg == "onehot":
            x = _ints(gen, (n, C), 1, 255) * (torch.randint(0, 2, (n, C), generator=gen).float() * 2 - 1)
        else:
            continue
        a = dict(op=c.op, x=x, logit=None, eps=1e-12)
        if lg == "const":
            a["logit"] = torch.full((n, C), 3.25) * torch.tensor([1.0, -1.0, 0.0, 30.0, -3e4])[None, :]
        elif lg == "wide":
            a["logit"] = torch.randn(n, C, generator=gen) * torch.tensor([1.0, 8.0, 100.0, 1e4, 1e4])[None, :]
        elif lg == "onehot":
            hot = torch.tensor([0, n - 1, n // 2, min(63, n - 1), min(64, n - 1)])
            a["logit"] = torch.zeros(n, C)
            a["logit"][hot, torch.arange(C)] = 80.0
            # the frame's own value, and the floored deviation: the root of eps as f32 arithmetic gives it, squared in f64 by the comparison
            want = torch.stack([x[hot, torch.arange(C)].double(), torch.full((C,), 1e-12).sqrt().double() ** 2])
            yield Launch("onehot", "exact", a, want, None, valid, None)
            continue
        ref, norm = stats_eval(a, torch.float64)
        if fam == "uniform":                                            # the mean is a quotient of integers; the deviation is not, it stays with `wide`
            mean_only = torch.stack([torch.ones(C, dtype=torch.bool), torch.zeros(C, dtype=torch.bool)])
            yield Launch(fam, fam, a, ref, None, mean_only, ~mean_only)
        else:
            yield Launch(fam, fam, a, ref, norm, valid, None)


# =======================================================================================================================================
# VQ: codebook lookup + projection, nearest-code search
# =======================================================================================================================================
def vq_cases():
    cs = [_case("vq_project", f"K{K}-cd{cd}-H{H}", K=K, cd=cd, H=H) for K, cd, H in ((1, 1, 1), (8192, 8, 255), (8192, 16, 256), (8192, 8, 257), (1, 16, 257))]
    cs += [_case("vq_search", f"ties-K{K}-cd{cd}-H{H}", K=K, cd=cd, H=H, kind="ties")
           for K, cd, H in ((1, 1, 1), (255, 1, 255), (256, 8, 256), (257, 1, 257), (8192, 1, 1024), (8192, 8, 1024), (257, 16, 255), (8192, 16, 257))]
    cs += [_case("vq_search", f"random-K{K}-cd{cd}-H{H}", K=K, cd=cd, H=H, kind="random")
           for K, cd, H in ((8192, 8, 1024), (257, 16, 255), (256, 8, 1), (255, 8, 256), (1, 8, 257))]      # (cd = 1 is all ties: the other family)
    return cs


def vq_project_eval(a, dt, mutant=None):
    e = a["codebook"].to(dt)[a["codes"]]
    w = a["w"].to(dt)
    return e @ w.T + a["bias"].to(dt), e.abs() @ w.abs().T + a["bias"].to(dt).abs()


def vq_search_scores(a, dt):
    z = a["h"].to(dt) @ a["w_in"].to(dt).T + a["b_in"].to(dt)
    e = z / z.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    cb = a["cb_norm"].to(dt)
    return -(((e * e).sum(-1, keepdim=True) - 2 * e @ cb.T) + a["cb_sq"].to(dt)[None, :])


def vq_search_eval(a, dt, mutant=None):
    s = vq_search_scores(a, dt)
    if mutant == "vq:tie_to_highest":
        K = s.shape[1]
        return (K - 1 - torch.flip(s, [1]).argmax(1)), None
    K = s.shape[1]
    best = s.max(1, keepdim=True).values
    return torch.where(s == best, torch.arange(K)[None, :], torch.full((), K)).min(1).values, None       # the first index of the maximum


def vq_margin(a):
    s = vq_search_scores(a, torch.float64)
    if s.shape[1] == 1:
        return torch.full((s.shape[0],), math.inf, dtype=torch.float64)
    top = torch.topk(s, 2, dim=1).values
    return top[:, 0] - top[:, 1]


TIE_SETS = ((0,), (255, 256), (256, 257), (63, 64), (44, 300), (1, 65, 129, 193), (255,), (-1,), (0, -1), (256, -1), (511, 512, 8191))


def vq_launches(c, families=("exact", "wide", "index")):
    p = P(c)
    K, cd, H = p["K"], p["cd"], p["H"]
    gen = _gen(c, 1)
    if c.op == "vq_project":
        n = 9
        codes = torch.randint(0, K, (n,), generator=gen)
        codes[0], codes[-1], codes[4] = 0, K - 1, K - 1
        for fam in families:
            if fam == "exact":
                a = dict(codes=codes, codebook=_ints(gen, (K, cd), -8, 8), w=_quarters(gen, (H, cd), 2), bias=_quarters(gen, (H,), 8))
            elif fam == "wide":
                a = dict(codes=codes, codebook=_lognormal(gen, (K, cd)), w=torch.randn(H, cd, generator=gen), bias=_lognormal(gen, (H,)))
            else:
                continue
            a.update(K=K, cd=cd, H=H)
            ref, norm = vq_project_eval(a, torch.float64)
            yield Launch(fam, fam, a, ref, norm if fam == "wide" else None, torch.ones(n, H, dtype=torch.bool), None)
        return
    if p["kind"] == "ties":
        if "exact" not in families:
            return
        # signed unit vectors: class 2 d + (sign < 0).  w_in[d][c] = (c % cd == d), the row's only nonzero input +-2 sits at a column of its class,
        # so z_e = +-2 e_d, e = +-e_d and every score is 0 (the class), -2 (orthogonal) or -4 (the opposite) exactly
        ncls = 2 * cd
        sets = [tuple(sorted({i % K for i in s})) for s in TIE_SETS if max(s) < K]
        per = max(1, ncls - 1)
        for l0 in range(0, len(sets), per):
            chunk = sets[l0:l0 + per]
            filler = ncls - 1                                           # the class every other index holds; a row of it must return the lowest such index
            cls = torch.full((K,), filler)
            for ci, s in enumerate(chunk):
                if ci < filler:
                    cls[list(s)] = ci
            rows_cls = [r for r in list(range(min(len(chunk), filler))) + [filler] if bool((cls == r).any())]
            cb = torch.zeros(K, cd)
            cb[torch.arange(K), cls // 2] = 1.0 - 2.0 * (cls % 2).float()
            h = torch.zeros(len(rows_cls), H)
            for i, r in enumerate(rows_cls):
                d = r // 2
                ncol = (H - d + cd - 1) // cd                           # the columns of class d: d, d + cd, ... (the tables keep H >= cd)
                h[i, d + cd * ((i * 37 + ncol - 1) % ncol)] = 2.0 * (1 - 2 * (r % 2))
            w_in = (torch.arange(H)[None, :] % cd == torch.arange(cd)[:, None]).float()
            a = dict(h=h, w_in=w_in, b_in=torch.zeros(cd), cb_norm=cb, cb_sq=(cb * cb).sum(1), K=K, cd=cd, H=H)
            want = torch.tensor([int((cls == r).nonzero()[0]) for r in rows_cls])
            yield Launch(f"ties#{l0 // per}", "exact", a, want.double(), None, torch.ones(len(rows_cls), dtype=torch.bool), None)
        return
    if "index" not in families:
        return
    n = 512
    cb = torch.randn(K, cd, generator=gen)
    cb = cb / cb.norm(dim=1, keepdim=True)
    h = torch.randn(n, H, generator=gen)
    h[7] = 0                                                            # a zero input row: z_e = b_in
    a = dict(h=h, w_in=torch.randn(cd, H, generator=gen) / math.sqrt(H), b_in=torch.randn(cd, generator=gen) * 0.1, cb_norm=cb, cb_sq=(cb * cb).sum(1),
             K=K, cd=cd, H=H)
    ref, _ = vq_search_eval(a, torch.float64)
    yield Launch("random", "index", a, ref.double(), vq_margin(a), torch.ones(n, dtype=torch.bool), None)


# =======================================================================================================================================
# the sinc resampler
# =======================================================================================================================================
RESAMPLE_RATIOS = ((3, 2), (2, 3), (160, 147), (441, 160), (3, 1))


def resample_table(orig, new):
    """The engine's own tap table (f32 [new][2 width + orig]) and its width: what indextts_amd.audio.Resample hands the kernel (host code, numpy)."""
    from indextts_amd.audio import sinc_kernel
    k, width, o, n = sinc_kernel(orig, new, 6, 0.99)
    assert (o, n) == (orig, new)
    return torch.from_numpy(np.ascontiguousarray(k)), int(width)


def resample_full(L_in, orig, new):
    """the largest L_out itts_resample_forward accepts"""
    return (L_in + orig - 1) // orig * new + new


def resample_eval(a, dt, mutant=None):
    x, kern = a["x"][:, :a["L_in"]].to(dt), a["kernel"].to(dt)
    B, L = x.shape
    orig, new, width = a["orig"], a["new"], a["width"]
    taps = 2 * width + orig
    nblk = (a["L_out"] + new - 1) // new
    xp = torch.zeros(B, width + max(L, nblk * orig) + taps, dtype=dt)
    xp[:, width:width + L] = x
    win = xp.unfold(1, taps, orig)[:, :nblk]                           # [B][nblk][taps]: x[i orig - width + j]
    y = torch.einsum("bij,pj->bip", win, kern).reshape(B, nblk * new)[:, :a["L_out"]]
    ny = torch.einsum("bij,pj->bip", win.abs(), kern.abs()).reshape(B, nblk * new)[:, :a["L_out"]]
    return y, ny


def resample_cases():
    return [_case("resample", f"{o}to{n}", orig=o, new=n) for o, n in RESAMPLE_RATIOS]


def resample_launches(c, families=("exact", "wide")):
    p = P(c)
    orig, new = p["orig"], p["new"]
    kern, width = resample_table(orig, new)
    for L_in in sorted({1, max(orig - 1, 1), orig, orig + 1, 1000}):
        full = resample_full(L_in, orig, new)
        for L_out in sorted({1, -(-new * L_in // orig), full}):
            B, xs, ys = 2, L_in + 5, L_out + 3
            valid = torch.zeros(B, ys, dtype=torch.bool)
            valid[:, :L_out] = True
            base = dict(kernel=kern, L_in=L_in, L_out=L_out, orig=orig, new=new, width=width, B=B, x_stride=xs, y_stride=ys)

            def framed(body):
                x = torch.full((B, xs), NAN)                            # the waveform past L_in within the row stride: never read
                x[:, :L_in] = body
                return x

            def out_framed(t):
                o = torch.full((B, ys), NAN, dtype=torch.float64)
                o[:, :L_out] = t
                return o
            if "exact" in families and L_out == full:
                for s in sorted({0, 1, orig - 1, orig, L_in - 1}):
                    if 0 <= s < L_in:
                        body = torch.zeros(B, L_in)
                        body[0, s] = 1.0
                        body[1, L_in - 1 - s] = -2.0
                        a = dict(base, x=framed(body))
                        ref, _ = resample_eval(a, torch.float64)        # an impulse: every output is one tap (times 1 or -2) or 0, exactly
                        yield Launch(f"impulse@{s}-Lin{L_in}-Lout{L_out}", "exact", a, out_framed(ref), None, valid, None)
            if "wide" in families:
                gen = _gen(c, L_in * 7 + L_out)
                a = dict(base, x=framed(_lognormal(gen, (B, L_in)) + 3.0))
                ref, norm = resample_eval(a, torch.float64)
                yield Launch(f"wide-Lin{L_in}-Lout{L_out}", "wide", a, out_framed(ref), out_framed(norm), valid, None)


# =======================================================================================================================================
# the framed-spectrum kernel (in-LDS Stockham FFT + mel bank)
# =======================================================================================================================================
FLT_EPSILON = 2.0 ** -23
#                name           n_fft  FL   hop  pad  mels bank      dc pre   pow layout floor        scale    n_samples
FBANK_CONFIGS = (("kaldi",        512,  400, 160,   0,  80, "kaldi",  1, 0.97, 2, 0, FLT_EPSILON, 32768.0, (399, 400, 1847)),     # 0, 1, 10 frames
                 ("mel",         1024, 1024, 256, 384,  80, "slaney", 0, 0.0,  1, 1, 1e-5,        1.0,     (385, 3000)),          # n = pad + 1: both sides reflect
                 ("n64-hop1",      64,   64,   1,   0,   1, "rand",   0, 0.97, 2, 0, 0.0,         1.0,     (64, 70)),
                 ("n64-fl2",       64,    2,   1,   0,   3, "rand",   1, 0.97, 1, 1, 1e-5,        1.0,     (2, 9)),
                 ("n2048",       2048, 2048, 256, 896,   5, "rand",   1, 0.0,  2, 1, 0.0,         1.0,     (897, 2500)),
                 ("n512-reflect", 512,  512, 256, 128,   4, "rand",   0, 0.97, 1, 0, 1e-5,        1.0,     (129, 1000)),
                 ("n1024-m100",  1024, 1024, 160, 432, 100, "rand",   0, 0.0,  2, 0, 1e-5,        1.0,     (433, 2000)))


def fbank_cases():
    keys = "n_fft FL hop pad n_mels bank remove_dc preemph power layout floor scale n_samples".split()
    return [_case("fbank", row[0], **dict(zip(keys, row[1:]))) for row in FBANK_CONFIGS]


def fbank_frames(FL, hop, pad, n):
    return 0 if n + 2 * pad < FL else 1 + (n + 2 * pad - FL) // hop


def fbank_tables(c):
    """(window [FL], twiddle [n_fft / 2][2], mel [n_mels][n_fft / 2 + 1]) f32: the engine's own host-built tables for the two production
    configurations, a random non-negative bank with ragged supports (the Nyquist bin among them) otherwise."""
    from indextts_amd import audio
    p = P(c)
    N, FL, M = p["n_fft"], p["FL"], p["n_mels"]
    tw = torch.from_numpy(audio.twiddles(N))
    if p["bank"] == "kaldi":
        return torch.from_numpy(audio.window_povey(FL)), tw, torch.from_numpy(audio.mel_banks_kaldi(M, N, 16000.0))
    win = torch.from_numpy(audio.window_hann_periodic(FL)) if FL > 2 else torch.tensor([0.75, 0.5])
    if p["bank"] == "slaney":
        return win, tw, torch.from_numpy(audio.mel_basis_slaney(22050, N, M, 0.0, None))
    gen = _gen(c, 99)
    nf = N // 2 + 1
    f = torch.arange(nf)[None, :]
    lo = torch.randint(0, nf - 1, (M, 1), generator=gen)
    hi = (lo + torch.randint(1, 70, (M, 1), generator=gen)).clamp(max=nf)
    hi[-1], lo[0] = nf, 0                                               # the last filter reaches the Nyquist bin, the first starts at DC
    mel = torch.rand(M, nf, generator=gen) * ((f >= lo) & (f < hi))
    return win, tw, mel


def fbank_eval(a, dt, mutant=None):
    FL, hop, N, pad, n = a["FL"], a["hop"], a["n_fft"], a["pad"], a["n_samples"]
    frames = fbank_frames(FL, hop, pad, n)
    B = a["B"]
    full = torch.full((B, a["out_stride"]), NAN, dtype=dt)
    if frames == 0:
        return full, full.clone()
    w = a["wave"][:, :n].to(dt) * a["scale"]
    s = torch.arange(frames)[:, None] * hop - pad + torch.arange(FL)[None, :]
    if mutant == "fbank:reflect_off_by_one":                            # the edge-repeating reflection
        s = torch.where(s < 0, -s - 1, s)
        s = torch.where(s >= n, 2 * n - 1 - s, s)
    else:
        s = torch.where(s < 0, -s, s)
        s = torch.where(s >= n, 2 * (n - 1) - s, s)
    fr = w[:, s.clamp(0, n - 1)]                                        # [B][frames][FL]
    win, c = a["window"].to(dt), a["preemph"]

    def dc(x):
        return x - x.mean(-1, keepdim=True) if a["remove_dc"] else x

    def pre(x):                                                         # y[i] = x[i] - c x[i - 1], the first sample against itself
        first = torch.zeros_like(x[..., :1]) if mutant == "fbank:preemph_zero_edge" else x[..., :1]
        return x - c * torch.cat([first, x[..., :-1]], -1) if c else x
    if mutant == "fbank:dc_after_preemph":
        fr = dc(pre(fr)) * win
    elif mutant == "fbank:window_before_dc":
        fr = pre(dc(fr * win))
    else:
        fr = pre(dc(fr)) * win
    X = torch.fft.rfft(torch.nn.functional.pad(fr, (0, N - FL)))
    mag2 = X.real * X.real + X.imag * X.imag
    Pw = mag2 if a["power"] == 2 else (mag2 + a["mag_eps"]).sqrt()
    mel = a["mel"].to(dt)
    lin = Pw @ mel.T                                                    # [B][frames][n_mels]
    absX = mag2.sqrt()
    R = (mag2.mean(-1, keepdim=True)).sqrt()                            # the frame's rms magnitude over the bins
    norm = (((absX + R) * R) @ mel.abs().T) if a["power"] == 2 else R * mel.abs().sum(1)[None, None, :]
    out = lin.clamp(min=a["floor"])
    if a["take_log"]:                                                   # d log = d lin / lin; the log's own f32 rounding is |log| u
        norm = norm / out + out.log().abs()
        out = out.log()
    M, ld = a["n_mels"], a["ld_out"]
    nfull = full.clone()
    if a["layout"] == 0:
        full[:, :frames * ld].view(B, frames, ld)[:, :, :M] = out
        nfull[:, :frames * ld].view(B, frames, ld)[:, :, :M] = norm
    else:
        full[:, :M * ld].view(B, M, ld)[:, :, :frames] = out.transpose(1, 2)
        nfull[:, :M * ld].view(B, M, ld)[:, :, :frames] = norm.transpose(1, 2)
    return full, nfull


def fbank_launches(c, families=("wide",)):
    if "wide" not in families:
        return
    p = P(c)
    win, tw, mel = fbank_tables(c)
    B = 2
    for n in p["n_samples"]:
        frames = fbank_frames(p["FL"], p["hop"], p["pad"], n)
        gen = _gen(c, n)
        wave = torch.full((B, n + 7), NAN)                              # the waveform past n_samples within the row stride: never read
        env = torch.exp(torch.cumsum(torch.randn(B, n, generator=gen) * 0.05, 1))
        wave[:, :n] = (0.05 * env / env.amax(1, keepdim=True) * torch.randn(B, n, generator=gen) * torch.exp(torch.randn(B, n, generator=gen))
                       + torch.tensor([[0.05], [-0.2]])).clamp(-1, 1)
        ld = (p["n_mels"] if p["layout"] == 0 else max(frames, 1)) + 3
        stride = (max(frames, 1) if p["layout"] == 0 else p["n_mels"]) * ld + 5
        for take_log in (0, 1):
            a = dict(wave=wave, window=win, twiddle=tw, mel=mel, B=B, n_samples=n, wave_stride=n + 7, ld_out=ld, out_stride=stride, take_log=take_log,
                     mag_eps=1e-9 if p["power"] == 1 else 0.0, **{k: p[k] for k in ("n_fft", "FL", "hop", "pad", "n_mels", "remove_dc", "preemph", "power",
                                                                                   "layout", "floor", "scale")})
            ref, norm = fbank_eval(a, torch.float64)
            yield Launch(f"n{n}-frames{frames}-log{take_log}", "wide", a, ref, norm, ~torch.isnan(ref), None)


# =======================================================================================================================================
# the table of ops
# =======================================================================================================================================
Op = collections.namedtuple("Op", "cases launches evaluate")
OPS = {
    "layernorm": Op(ln_cases, ln_launches, ln_eval),
    "attention": Op(attn_cases, attn_launches, attn_eval),
    "gelu": Op(None, point_launches, point_eval), "glu": Op(None, point_launches, point_eval), "act": Op(None, point_launches, point_eval),
    "gate": Op(None, point_launches, point_eval), "scale_residual": Op(None, point_launches, point_eval), "affine": Op(None, point_launches, point_eval),
    "dwconv": Op(dwconv_cases, dwconv_launches, dwconv_eval),
    "gather_conv": Op(gather_cases, gather_launches, gather_eval),
    "groupnorm_mish": Op(gn_cases, gn_launches, gn_eval),
    "l2norm": Op(l2_cases, l2_launches, l2_eval),
    "colnorm": Op(colnorm_cases, colnorm_launches, colnorm_eval),
    "ctxpool": Op(ctx_cases, ctx_launches, ctx_eval),
    "statspool": Op(None, stats_launches, stats_eval), "attnstats": Op(None, stats_launches, stats_eval),
    "vq_project": Op(None, vq_launches, vq_project_eval), "vq_search": Op(None, vq_launches, vq_search_eval),
    "resample": Op(resample_cases, resample_launches, resample_eval),
    "fbank": Op(fbank_cases, fbank_launches, fbank_eval),
}
CASES = (ln_cases() + attn_cases() + point_cases() + dwconv_cases() + gather_cases() + gn_cases() + l2_cases() + colnorm_cases() + ctx_cases() +
         stats_cases() + vq_cases() + resample_cases() + fbank_cases())


def launches(c, families=("exact", "uniform", "wide", "index")):
    return OPS[c.op].launches(c, families)


POOLS = ("statspool", "attnstats")


def evaluate(c, lch, dt=torch.float64, mutant=None):
    """The op's definition on a launch's operands in `dt` (with a named defect), in the form the engine returns it: f32 (int64 indices for the
    VQ search), the pooling ops' variance as its f32 root, framed like lch.ref with NaN outside what the op writes."""
    out, _ = OPS[c.op].evaluate(lch.args, dt, mutant)
    if c.op == "vq_search":
        return out
    out = out.float()
    if c.op in POOLS:
        out = torch.stack([out[0], out[1].sqrt()])
    if out.shape != lch.ref.shape:                                      # outputs framed by a wider leading dimension (colnorm, resample)
        full = torch.full(lch.ref.shape, NAN)
        full[..., :out.shape[-1]] = out
        out = full
    return out


def compared(c, out):
    """What is compared, in f64: the deviation the pooling ops return is squared (the variance is compared, not its root)."""
    out = out.double()
    return torch.stack([out[0], out[1] * out[1]]) if c.op in POOLS else out


def error_over_norm(c, lch, out):
    """largest |out - ref| / normaliser over the valid elements of a wide launch (inf where the normaliser is 0 and the output differs)"""
    err = (compared(c, out) - lch.ref).abs()[lch.valid]
    r = torch.where(err == 0, torch.zeros((), dtype=torch.float64), err / lch.norm[lch.valid])
    return float(torch.nan_to_num(r, nan=math.inf).max()) if r.numel() else 0.0


@functools.lru_cache(maxsize=None)
def baseline_E(op, name=None):
    """E(op): the largest elementwise error of the plain-f32 evaluation against f64 over the op's wide launches, in units of the normaliser.
    With a case name: over that case's launches alone (the framed spectrum: one configuration's FFT length and bank are one case, each with
    hundreds of outputs, and a bank that lets one dominant bin through would otherwise set the limit of every other configuration)."""
    E = 0.0
    for c in CASES:
        if c.op == op and name in (None, c.name):
            for lch in launches(c, ("wide",)):
                E = max(E, error_over_norm(c, lch, evaluate(c, lch, torch.float32)))
    return E


def E_of(c):
    return baseline_E(c.op, c.name) if c.op == "fbank" else baseline_E(c.op)


# =======================================================================================================================================
# the comparison both files apply (an empty list = the output passes)
# =======================================================================================================================================
def check(c, lch, out, stats=None):
    """out: the engine's output shaped like lch.ref (f32; int64 indices for vq_search); the canaries outside lch.valid are the caller's.
    stats: a dict that receives ratio = largest error / limit and E (wide family)."""
    valid = lch.valid
    if c.op == "vq_search":
        got, want = out.long()[valid], lch.ref.long()[valid]
        if lch.family == "exact":
            bad = (got != want).nonzero().flatten()
            return [f"{bad.numel()} of {want.numel()} rows miss the lowest index of their maximum; first row {int(bad[0])}: {int(got[bad[0]])} vs "
                    f"{int(want[bad[0]])}"] if bad.numel() else []
        held = lch.norm > VQ_MARGIN
        bad = ((got != want) & held).nonzero().flatten()
        fails = [f"{bad.numel()} rows with an f64 margin above {VQ_MARGIN} differ from the f64 argmax; first row {int(bad[0])}: {int(got[bad[0]])} vs "
                 f"{int(want[bad[0]])}"] if bad.numel() else []
        if float((~held).float().mean()) > VQ_EXEMPT_SHARE:
            fails.append(f"{int((~held).sum())} of {held.numel()} rows are exempt")
        return fails
    if bool(torch.isnan(out[valid]).any()):
        return [f"{int(torch.isnan(out[valid]).sum())} of {int(valid.sum())} valid elements are NaN (never written, or a poisoned input was read)"]
    got = compared(c, out)
    if lch.family == "exact":
        want = lch.ref if c.op in POOLS else lch.ref.float().double()
        bad = ((got.view(torch.int64) != want.view(torch.int64)) & valid).nonzero()
        if bad.shape[0]:
            i = tuple(bad[0].tolist())
            return [f"{bad.shape[0]} of {int(valid.sum())} elements differ bitwise from the exact result; first at {list(i)}: {float(got[i])!r} vs {float(want[i])!r}"]
        return []
    if lch.family == "uniform":
        err = (got - lch.ref).abs()
        bad = (~(err <= 2 * f32_ulp(lch.ref)) & valid).nonzero()
        if bad.shape[0]:
            i = tuple(bad[0].tolist())
            return [f"{bad.shape[0]} of {int(valid.sum())} elements are more than 2 ulp off the f64 quotient; first at {list(i)}: {float(got[i])!r} vs "
                    f"{float(lch.ref[i])!r}"]
        return []
    E = E_of(c)
    r = error_over_norm(c, lch, out)
    ratio = (0.0 if r == 0 else math.inf) if E == 0 else r / (MARGIN * E)
    if stats is not None:
        stats.update(ratio=ratio, E=E)
    return [f"largest error / limit = {ratio:.3f} (E = {E:.3e})"] if not ratio <= 1.0 else []


# every named wrong variant: the op whose evaluate() knows it
MUTANTS = {
    "attn:first-1": "attention", "attn:first+1": "attention", "attn:last+1": "attention", "attn:last-1": "attention",
    "attn:drop@63": "attention", "attn:drop@64": "attention", "attn:drop@last": "attention",
    "rel:sign": "attention", "rel:left_clamp": "attention", "rel:right_clamp": "attention", "rel:no_clamp": "attention",
    "ln:unbiased_variance": "layernorm", "ln:eps_outside_root": "layernorm", "ln:one_pass_variance": "layernorm",
    "gn:unbiased_variance": "groupnorm_mish", "gn:eps_outside_root": "groupnorm_mish",
    "colnorm:ddof_swapped": "colnorm", "colnorm:eps_outside_root": "colnorm",
    "statspool:biased_variance": "statspool", "attnstats:unbiased_variance": "attnstats",
    "ctxpool:last_segment_by_seg_len": "ctxpool", "dwconv:padding": "dwconv", "gather:exact_floor": "gather_conv",
    "vq:tie_to_highest": "vq_search", "gelu:tanh_form": "gelu",
    "fbank:reflect_off_by_one": "fbank", "fbank:preemph_zero_edge": "fbank", "fbank:dc_after_preemph": "fbank", "fbank:window_before_dc": "fbank",
}
