"""What the alignment-export tests share (tests/test_gpu_align_matrix.py, tests/test_gpu_alignment.py, tests/test_alignment_host.py): the unit
cases of `itts_gpt_attention_align_forward`, an f64 reference written from the entry's definition with its first-order error bound, and an f64
restatement of the GPT-2 stack that returns its softmax weights.  No GPU import.

The definition (include/indextts_hip.h: itts_gpt_attention_align_forward).  For dense row b and the i-th listed head hd:

    pb    = seq_map[b] if given, else b * max(seq_mul, 1)          physical cache row; entry of pad and pos_shift
    last  = min(pos - shift[pb], Tmax - 1),   first = pad[pb]
    u     = row_slot[b] if given, else b;     rstep = step - row_step0[u];     (off, len) = span[u]
    out[u][rstep][i][j] = softmax over t in [first, last] of q[b][hd] . K[pb][hd][t] / 8, at t = first + off + j, j < len; 0 past `last`

and nothing at all is written for a row with finished[u], rstep < 0, rstep >= max_new or rstep >= row_limit[u].

The bound (`bound`), first order, per exported element -- derived as `hilo_term` of tests/attn_matrix.py derives its own, from the kernel's
arithmetic and not from its output.  u = 2^-24 (f32 unit round-off).
  scores:  a lane runs one fma chain over its 64 / LPK dims and the LPK lanes of a key are summed by an xor-shuffle tree of log2(LPK) adds: a
           sum of 64 products evaluated with at most DEPTH = 8 + 3 = 11 (bf16 cache, LPK = 8) / 4 + 4 = 8 (f32 cache, LPK = 16) roundings on any
           path, so |s_t - exact| <= DEPTH u A_t (1 + O(u)), A_t = sum_j |q_j| |k_tj| / 8 (the scaling by 1/8 is exact).  A score error e_t moves
           p_t = exp(s_t) / sum_v exp(s_v) by p_t (e_t - sum_v p_v e_v) to first order: at most p_t DEPTH u (A_t + sum_v p_v A_v).
  exp:     the argument s_t - max is rounded once (u |s_t - max| absolute, which is a RELATIVE error of e_t), expf is taken as accurate to
           2 ulp (2^-22 relative; the device library documents 1 ulp): E_t = 2^-22 + u |s_t - max|; the sum runs in f64 over these e_t, so p_t
           moves by at most p_t (E_t + sum_v p_v E_v).
  output:  one f64 division rounded to f32: p_t u; results below the smallest normal f32 may flush: + 2^-126.
  second order: every relative term above is below 1e-4 for these operands, so the squares are below 1e-8 of the first order; the bound is
           multiplied by 1 + 1e-3 to cover them."""
import collections
import math
import zlib

import torch

PREC_F32, PREC_BF16 = 0, 1
H, HD, ROWS, UTTS, MAX_NEW = 4, 64, 8, 5, 6
D = H * HD
SENTINEL = -7.0
U = 2.0 ** -24
DEPTH = {PREC_F32: 8, PREC_BF16: 11}
SECOND_ORDER = 1.0 + 1e-3

WINDOWS = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)      # 256 / 512: the f32 / bf16 pass width
PADS = (0, 15, 64, 65)
SPAN_KINDS = ("head", "mid", "tail", "past", "empty", "full")
WRITTEN_KINDS = tuple(k for k in SPAN_KINDS if k != "empty")
HEAD_SETS = ((0,), (H - 1,), (H - 1, 1))

Case = collections.namedtuple("Case", "name prec Tmax pos pad shift seq_map row_slot step row_step0 row_limit finished spans heads cap expect")
# pad, shift: ROWS entries or None; seq_map, row_slot: 3 entries or None; row_step0, row_limit, finished: UTTS entries or None; spans: UTTS
# (off, len); expect: per dense row whether it writes


def span_of(kind, n, cap):
    """(off, len) of a span kind over a window of n keys with rows of `cap` columns"""
    if kind == "head":
        return 0, 1
    if kind == "mid":
        return max(1, n // 3), min(cap, 5)                  # off > 0; 5: not a multiple of 4 (runs past `last` in the shortest windows)
    if kind == "tail":
        ln = min(n, min(cap, 7))
        return n - ln, ln                                   # ends exactly at `last`
    if kind == "past":
        return max(0, n - 2), min(cap, 6)                   # the last two keys, then zeros
    if kind == "far":
        return 2 ** 31 - 3, min(cap, 5)                     # starts far past `last` (off + j would overflow an int): all zeros
    if kind == "empty":
        return 3, 0                                         # nothing written
    return 0, cap                                           # len = text_cap


def case_id(c):
    return f"{'bf16' if c.prec else 'f32'}-{c.name}"


def _build():
    cases = []

    def add(name, prec, windows, i, cap=16, pos_over=0, skip=None, kinds=None):
        """three dense rows with the given window lengths; tables by the bits of i"""
        seq_map = (4, 0, 2) if i & 1 else None
        pbs = list(seq_map) if seq_map else [0, 1, 2]
        use_shift, use_slot, use_step0 = bool(i & 2), bool(i & 4) or bool(i & 1), bool(i & 2)
        firsts = [PADS[(i + j) % 4] for j in range(3)]
        if i % 3 == 0:
            firsts = None if all(f == 0 for f in firsts) else firsts
        f3 = firsts or [0, 0, 0]
        lasts = [f + n - 1 for f, n in zip(f3, windows)]
        pos = max(lasts)
        shifts = [pos - l for l in lasts]
        if not use_shift and any(shifts):                   # without the table every row ends at `pos`: move the pads instead
            f3 = [pos - n + 1 for n in windows]
            if min(f3) < 0:
                pos -= min(f3)
                f3 = [pos - n + 1 for n in windows]
            shifts = [0, 0, 0]
        Tmax = pos + 3
        pad = [min(2 + r, Tmax - 1) for r in range(ROWS)]
        shift = [min(1 + r, pos) for r in range(ROWS)]
        for pb, f, s in zip(pbs, f3, shifts):
            pad[pb], shift[pb] = f, s
        if pos_over:                                        # the position counter past the cache row: every window ends at Tmax - 1
            Tmax = pos + 1
            pos += pos_over
            shift = None
        slot = (3, 0, 4) if use_slot else None
        us = list(slot) if slot else [0, 1, 2]
        step = 4 if use_step0 else 2
        step0 = [9] * UTTS
        for j, u in enumerate(us):
            step0[u] = (1, 3, 0)[j] if use_step0 else 0
        # (the rotation never hands out `empty`: every window of these cases is compared; `span-empty` below carries that kind)
        kinds = kinds or [WRITTEN_KINDS[(i + 2 * j) % len(WRITTEN_KINDS)] for j in range(3)]
        spans = [(1, 2)] * UTTS
        for u, k, n in zip(us, kinds, windows):
            spans[u] = span_of(k, n, cap)
        limit = fin = None
        expect = [True, True, True]
        if skip:
            fin, limit = [0] * UTTS, [MAX_NEW] * UTTS
            for j, why in enumerate(skip):
                rstep = step - step0[us[j]]
                if why == "finished":
                    fin[us[j]] = 1
                elif why == "limit":
                    limit[us[j]] = rstep                    # rstep >= the row's limit
                elif why == "limit+1":
                    limit[us[j]] = rstep + 1                # the last step the limit allows: written
                elif why == "max_new":
                    step0[us[j]] = step - MAX_NEW           # rstep == max_new
                elif why == "negative":
                    step0[us[j]] = step + 1
                expect[j] = why in (None, "limit+1")
        cases.append(Case(name, prec, Tmax, pos, tuple(pad) if (firsts or seq_map or any(f3)) else None, tuple(shift) if (use_shift and shift) else None,
                          seq_map, slot, step, tuple(step0) if (use_step0 or skip) else None, tuple(limit) if limit else None,
                          tuple(fin) if fin else None, tuple(spans), HEAD_SETS[i % 3], cap, tuple(expect)))

    for prec in (PREC_F32, PREC_BF16):
        for i in range(0, len(WINDOWS) - 2, 3):
            w = WINDOWS[i:i + 3]
            add("win-" + "-".join(map(str, w)), prec, w, i // 3)
        add("win-1023-1024-1025", prec, (1023, 1024, 1025), 7)
        add("win-511-512-513", prec, (511, 512, 513), 4)
        add("cap1024-full", prec, (1025, 1024, 257), 3, cap=1024, kinds=("full", "full", "full"))
        add("clamp", prec, (65, 9, 130), 5, pos_over=11)
        add("span-empty", prec, (65, 9, 130), 1, kinds=("empty", "far", "mid"))
        # the surviving row of either case has a span with keys in it: a kernel that left every block would fail here
        add("skip-finished-limit", prec, (65, 9, 130), 6, skip=("finished", "limit", "limit+1"), kinds=("mid", "tail", "past"))
        add("skip-max_new-negative", prec, (5, 64, 129), 2, skip=("max_new", None, "negative"), kinds=("tail", "mid", "head"))
    return cases


CASES = _build()


def geometry(c):
    """per dense row: (pb, first, last, u, rstep, off, len)"""
    out = []
    for b in range(3):
        pb = c.seq_map[b] if c.seq_map else b
        first = c.pad[pb] if c.pad else 0
        last = min(c.pos - (c.shift[pb] if c.shift else 0), c.Tmax - 1)
        u = c.row_slot[b] if c.row_slot else b
        rstep = c.step - (c.row_step0[u] if c.row_step0 else 0)
        off, ln = c.spans[u]
        out.append((pb, first, last, u, rstep, off, min(ln, c.cap)))
    return out


def operands(c):
    """(q [3][D] f32, k [ROWS][H][Tmax][64] f32 holding the cache's values -- bf16-representable for the bf16 cache): scores of standard
    deviation 2.5; every cell outside the three windows is NaN"""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()))
    q = torch.randn(3, D, generator=gen) * 2.5
    k = torch.randn(ROWS, H, c.Tmax, HD, generator=gen)
    if c.prec == PREC_BF16:
        k = k.bfloat16().float()
    seen = torch.zeros(ROWS, c.Tmax, dtype=torch.bool)
    for pb, first, last, *_ in geometry(c):
        seen[pb, first:last + 1] = True
    return q, torch.where(seen[:, None, :, None], k, torch.full((), float("nan")))


def reference(c, q, k):
    """[(u, rstep, ref [n_heads][len] f64, bound [n_heads][len] f64)] of the rows that write, and `writes`: the (u, rstep) that must stay
    untouched are all the others"""
    rows = []
    for b, (pb, first, last, u, rstep, off, ln) in enumerate(geometry(c)):
        if not c.expect[b]:
            continue
        ref = torch.zeros(len(c.heads), ln, dtype=torch.float64)
        lim = torch.full((len(c.heads), ln), 2.0 ** -126, dtype=torch.float64)
        for i, hd in enumerate(c.heads):
            qq = q[b, hd * HD:(hd + 1) * HD].double()
            kk = k[pb, hd, first:last + 1].double()
            p, bd = softmax_with_bound(qq, kk, c.prec)
            hi = min(ln, max(0, last - first + 1 - off))
            ref[i, :hi] = p[off:off + hi]
            lim[i, :hi] += bd[off:off + hi]
        rows.append((u, rstep, ref, lim))
    return rows


def softmax_with_bound(q, k, prec):
    """p [n] f64 = softmax(k q / 8) and the first-order bound of the module docstring, elementwise"""
    s = k @ q / 8
    A = k.abs() @ q.abs() / 8
    p = torch.softmax(s, 0)
    E = 2.0 ** -22 + U * (s - s.max()).abs()
    d = DEPTH[prec] * U
    return p, SECOND_ORDER * p * (d * (A + (p * A).sum()) + (E + (p * E).sum()) + U)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the GPT-2 stack restated in f64, returning the softmax weights (tests/test_gpu_alignment.py teacher-forces the engine's own ids through it)
# ---------------------------------------------------------------------------------------------------------------------------------------
def gelu_new(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def layer_norm(x, g, b, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def stack_attention(sd, layers, heads, x, pad, pairs, eps=1e-5):
    """One causal pass of the GPT-2 blocks `gpt.h.*` of state dict `sd` over x (T, D) in f64, keys left of `pad` masked out.  Returns
    {(layer, head): (T, T) f64 softmax weights} for `pairs` (row = query position, column = key position)."""
    f = lambda name: sd[name].double()
    x = x.double()
    T, Dm = x.shape
    dh = Dm // heads
    t = torch.arange(T)
    allowed = (t[None, :] <= t[:, None]) & (t[None, :] >= pad)
    out = {}
    for l in range(layers):
        p = f"gpt.h.{l}."
        h = layer_norm(x, f(p + "ln_1.weight"), f(p + "ln_1.bias"), eps)
        qkv = h @ f(p + "attn.c_attn.weight") + f(p + "attn.c_attn.bias")
        q, k, v = (z.view(T, heads, dh).transpose(0, 1) for z in qkv.split(Dm, dim=1))
        s = q @ k.transpose(1, 2) / math.sqrt(dh)
        w = torch.softmax(torch.where(allowed[None], s, torch.full((), -math.inf, dtype=torch.float64)), -1)
        w = torch.nan_to_num(w, nan=0.0)                    # queries left of the pad see nothing
        for (pl, ph) in pairs:
            if pl == l:
                out[(pl, ph)] = w[ph]
        a = (w @ v).transpose(0, 1).reshape(T, Dm)
        x = x + a @ f(p + "attn.c_proj.weight") + f(p + "attn.c_proj.bias")
        h = layer_norm(x, f(p + "ln_2.weight"), f(p + "ln_2.bias"), eps)
        x = x + gelu_new(h @ f(p + "mlp.c_fc.weight") + f(p + "mlp.c_fc.bias")) @ f(p + "mlp.c_proj.weight") + f(p + "mlp.c_proj.bias")
    return out


def teacher_forced_alignment(sd, layers, heads, prefix, pad, ids, pairs, span, pos_offset=2):
    """What `generate(..., alignment_heads=pairs, text_spans=[span])` exports for ONE row, restated: prefix (S, D) = the engine's prompt of the
    row (cached prefix + start-mel row), pad = its left padding, ids = the codes the engine generated.  The query that predicts code i >= 1
    is the input row of code i - 1 -- mel_embedding[code] + mel_pos_embedding[i - 1 + pos_offset] -- at position S - 1 + i.  Returns
    (n, K, len) f64, row 0 zero."""
    S = prefix.shape[0]
    n = len(ids)
    me, mp = sd["mel_embedding.weight"].double(), sd["mel_pos_embedding.emb.weight"].double()
    rows = [me[int(ids[i - 1])] + mp[i - 1 + pos_offset] for i in range(1, n)]
    x = torch.cat([prefix.double()] + ([torch.stack(rows)] if rows else []), 0)
    w = stack_attention(sd, layers, heads, x, int(pad), pairs)
    off, ln = span
    out = torch.zeros(n, len(pairs), ln, dtype=torch.float64)
    for i in range(1, n):
        for k, pr in enumerate(pairs):
            out[i, k] = w[pr][S - 1 + i, pad + off: pad + off + ln]
    return out


def exhaustive_best_path(logp):
    """(best score, best path) over EVERY path j(0) = 0, j(n - 1) = T - 1, steps of 0 / +1, by enumeration (small matrices only)"""
    n, T = len(logp), len(logp[0])
    best = (-math.inf, None)

    def walk(i, j, score, path):
        nonlocal best
        score += logp[i][j]
        path = path + [j]
        if i == n - 1:
            if j == T - 1 and score > best[0]:
                best = (score, path)
            return
        walk(i + 1, j, score, path)
        if j + 1 < T:
            walk(i + 1, j + 1, score, path)
    walk(0, 0, 0.0, [])
    return best
