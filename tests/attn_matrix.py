"""The KV-cache attention test matrix shared by tests/test_gpu_attn_matrix.py (GPU) and tests/test_attn_matrix_host.py (CPU): the launches the
engine makes through `launch_attention` (the `run_layers` call sites of capi_gpt.hip) at the edges of the two kernels behind it, the kernel
and geometry each is meant for (by the name `itts_attention_last_path` reports), three families of operands, an f64 reference written from
the definition, and the comparisons both files apply.  No GPU import.

The definition (include/indextts_hip.h: itts_gpt_attention_forward).  For sequence b, head h, query qi:

    pb    = seq_map[b] if given, else b * max(seq_mul, 1)               physical cache row; entry of pad and pos_shift
    last  = min(pos + qi - shift[pb], Tmax - 1),   first = pad[pb]
    row_t = the row map chosen by the step's parity, [b][t], if given, else pb
    out   = softmax over t in [first, last] of q . K[row_t][h][t] / 8, times V[row_t][h][t];  0 when the window is empty

Every case has 2 heads (D = 128), 8 physical cache rows, and -- but for the one launch of more than 256 blocks -- 3 logical sequences.

Operands, per case (anything the bf16 engine stores holds bf16 values, so the reference sees the cache's real contents):

* one-hot -- q = 16 e_d; every key a query may see is 0 but for its target, which holds 20 at d: the target scores exactly 40, the others
  exactly 0, V holds integers of magnitude 1 .. 255, and the output must be the target's V row BITWISE (the other keys weigh n e^-40 in
  all, checked on the host against half an ulp).  The target sits in turn at first, first + 1, last - 1, last and at first + 63 / + 64 /
  + 1023 / + 1024 where the window has them (the 64-key chunk, the 16-stream wrap).  With several queries per sequence every distinct
  target position of a (sequence, head) takes a dimension of its own; 62 fit into a launch, further queries wait for the next launch and
  meanwhile aim at `first`.  Under the rule `last` the key behind a query's window (the next query's target) additionally scores 80
  against that query, so a causal edge off by one returns the wrong V row.
* uniform -- q = 0, V integers in 1 .. 255: the output is sum / n, an exact count of the keys (f32 engine: within 2 ulp of the f64 quotient,
  the MFMA kernel multiplies by a reciprocal; bf16 engine: within one bf16 step -- so at large n only the f32 engine resolves a miscount).
* random, wide range -- scores span about +-8, V elementwise log-normal magnitudes of either sign; held to the limit below.

Poison, detected by value: cache cells no query of the launch may see but that lie inside what the launch's tables name (keys left of
`first`, keys behind a query's own position, other named rows at the same positions) hold V = 1e30 and, in the one-hot family, a K row
scoring +80; cells behind a row's last written key and rows no table names hold NaN.  Every index of every table is in range.

The limit of the random family is measured on the reference side, never on the kernels: the same definition evaluated by torch in plain
f32 (matmul, softmax) has a largest elementwise error E against f64, normalised by sum_t w_t |v_td|; the f32 engine is held to 4 E (the
margin of test_layernorm_vs_torch: another accumulation order, not a worse one), the bf16 engine to 4 E plus one bf16 step of |ref| for
the rounding of its output.  The bf16 MFMA kernel alone gets one derived term more, for the 16-bit hi + lo pairs that carry its query and
its probabilities into the matrix pipe (hilo_term: derivation and what was measured)."""
import collections
import functools
import math
import zlib

import torch

PREC_F32, PREC_BF16 = 0, 1
H, HD, D, ROWS = 2, 64, 128, 8
MAP_ROWS = 6                 # the row maps name rows 0 .. 5; rows 6, 7 stay unnamed
NAN = float("nan")
POISON_V = 1e30
Q_HOT, K_HOT, K_POISON = 16.0, 20.0, 40.0        # 16 * 20 / 8 = 40 (the target), 16 * 40 / 8 = 80 (a key that must not be seen)
SLOTS = 62                   # dimensions for per-query targets in one launch; slot 62 is `first`'s

# every name itts_attention_path_name lists, in its order
ALL_PATHS = [f"streams_{p}_w{w}{r}" for p in ("f32", "bf16") for w in (4, 8, 16) for r in ("", "_rmap")] + ["prefill_mfma_f32", "prefill_mfma_bf16"]

Case = collections.namedtuple("Case", "name prec kind nseq nq Tmax pos pad shift seq_map seq_mul rmap step opts waves")
# kind: "streams" (attn_kernel) / "mfma" (attn_prefill_mfma_kernel); pad, shift: 8 entries (one per cache row) or None; seq_map: nseq entries or None;
# rmap: both row maps are passed, step is *step_ptr; opts: engine options of the launch; waves: the attn_waves settings it runs at (0 = by shape)

ONEHOT_RULES = ("first", "first+1", "last-1", "last", "first+63", "first+64", "first+1023", "first+1024")
KEY_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1088, 1089)
FIRSTS = (0, 1, 63, 64, 65)
MUTANTS = ("first-1", "last+1", "first+1", "last-1", "drop@first+63", "drop@first+64", "drop@first+1023", "drop@first+1024",
           "parity", "no_seq_map", "no_pos_shift", "heads")


def case_id(c):
    return f"{'bf16' if c.prec else 'f32'}-{c.kind}-{c.name}"


def path_of(c, waves):
    """The kernel and geometry the case is meant for at an attn_waves setting."""
    p = "bf16" if c.prec == PREC_BF16 else "f32"
    if c.kind == "mfma":
        return f"prefill_mfma_{p}"
    if waves == 0:
        waves = 4 if c.nq > 1 else 16 if c.nseq * H <= 256 else 8
    return f"streams_{p}_w{waves}" + ("_rmap" if c.rmap else "")


def _table(pbs, vals, filler):
    """An 8-entry per-cache-row table: vals at the rows the sequences use, `filler(r)` (in range, different) elsewhere."""
    t = [filler(r) for r in range(ROWS)]
    for r, v in zip(pbs, vals):
        t[r] = v
    return tuple(t)


def _build():
    cases = []

    def add(name, prec, kind, nq, Tmax, pos, pad=None, shift=None, seq_map=None, seq_mul=1, rmap=False, step=0, opts=None, waves=(0,), nseq=3):
        pbs = list(seq_map) if seq_map is not None else [b * max(seq_mul, 1) for b in range(nseq)]
        if pad is not None and len(pad) != ROWS:
            pad = _table(pbs, pad, lambda r: min(2 + r, Tmax - 1))
        if shift is not None and len(shift) != ROWS:
            shift = _table(pbs, shift, lambda r: min(1 + r, pos))
        if pad is not None:
            Tmax = max(Tmax, max(pad) + 2)                     # a pad is a position of the cache row, whether a query reaches it or not
        opts = dict(opts or {})
        if kind == "mfma":
            opts.setdefault("prefill_attn", 1)
        elif nq > 1 and prec == PREC_BF16:
            opts.setdefault("prefill_attn", 0)
        cases.append(Case(name, prec, kind, nseq, nq, Tmax, pos, pad, shift, tuple(seq_map) if seq_map is not None else None, seq_mul, rmap,
                          step, tuple(sorted(opts.items())), tuple(waves)))

    W = (4, 8, 16, 0)
    for prec in (PREC_F32, PREC_BF16):
        # ---- decode steps (nq = 1): the combinations decode_step and the beam step make, at every geometry and the default pick ----
        add("dec-plain", prec, "streams", 1, 77, 70, waves=W)
        add("dec-pad", prec, "streams", 1, 77, 70, pad=(0, 1, 65), waves=W)
        add("dec-seqmap", prec, "streams", 1, 77, 70, seq_map=(4, 0, 2), waves=W)
        add("dec-seqmap-pad-shift", prec, "streams", 1, 140, 133, pad=(5, 0, 64), shift=(64, 3, 0), seq_map=(4, 0, 2), waves=W)
        add("dec-shift", prec, "streams", 1, 140, 133, shift=(0, 3, 64), waves=W)
        for step in (0, 1):
            add(f"dec-rmap-step{step}", prec, "streams", 1, 77, 70, pad=(0, 1, 65), rmap=True, step=step, waves=W)
            add(f"dec-rmap-shift-step{step}", prec, "streams", 1, 140, 133, pad=(5, 0, 64), shift=(0, 3, 64), rmap=True, step=step, waves=W)
        # more than 256 blocks: 130 sequences x 2 heads take the 8-wave kernel by default (the sequences share three cache rows)
        add("dec-260-blocks", prec, "streams", 1, 40, 33, pad=_table((4, 0, 2), (0, 1, 5), lambda r: 2 + r), seq_map=[(4, 0, 2)[b % 3] for b in range(130)],
            nseq=130)
        # a finished row of a long-running session: the position is past the cache row, the window ends at Tmax - 1
        add("dec-clamp", prec, "streams", 1, 130, 140, pad=(0, 5, 70), waves=W)

        # ---- the key counts of the stream kernel, three per launch (different pad and shift per sequence), with and without the row map ----
        for i in range(8):
            ns = [KEY_COUNTS[j] if j < len(KEY_COUNTS) else KEY_COUNTS[j - 2] for j in (i, i + 8, i + 16)]
            firsts = [FIRSTS[(i + j) % 5] for j in range(3)]
            lasts = [f + n - 1 for f, n in zip(firsts, ns)]
            pos = max(lasts)
            for rmap in (False, True):
                add(f"keys-{ns[0]}-{ns[1]}-{ns[2]}" + ("-rmap" if rmap else ""), prec, "streams", 1, pos + 4, pos, pad=firsts,
                    shift=[pos - x for x in lasts], rmap=rmap, step=i & 1, waves=(4, 8, 16))

        # ---- the stream kernel with several queries per sequence (the f32 engine's prefill; prefill_attn = 0 in the bf16 engine) ----
        for nq in (2, 5, 65):
            add(f"pf-nq{nq}-pad", prec, "streams", nq, 70 + nq + 3, 70, pad=(0, 1, 65), waves=W)
        add("pf-nq5-seqmul3", prec, "streams", 5, 78, 70, pad=(3, 0, 64), seq_mul=3, waves=W)

        # ---- the MFMA kernel: 16-query wave edge, 64-query block edge, tile loop from `first`, V-tile clamp ----
        pads = (None, (0, 15, 64), (1, 16, 65), (17, 63, 0))        # every set keeps one sequence with keys at any pos0
        for i, nq in enumerate((2, 15, 16, 17, 63, 64, 65, 129)):
            for j, pos0 in enumerate((0, 1, 63, 64, 65, 200)):
                pad = pads[(i + j) % 4]
                add(f"mfma-nq{nq}-pos{pos0}-pad{'-'.join(map(str, pad)) if pad else 'none'}", prec, "mfma", nq, pos0 + nq + 3, pos0, pad=pad)
        add("mfma-long", prec, "mfma", 65, 1068, 1000, pad=(0, 65, 1001))
        add("mfma-pad-past-first-queries", prec, "mfma", 17, 21, 1, pad=(6, 0, 3))                   # sequence 0: queries 0 .. 4 see no key
        add("mfma-seqmul3", prec, "mfma", 17, 84, 64, pad=(3, 0, 64), seq_mul=3)
        add("mfma-shift", prec, "mfma", 17, 220, 200, shift=(0, 3, 64))                              # the latent session's append
    # the bf16 engine's own pick for S > 1 is the MFMA kernel, the f32 engine's the stream kernel at 4 waves
    add("mfma-default-pick", PREC_BF16, "mfma", 17, 84, 64, pad=(3, 0, 64), opts={"prefill_attn": -1})
    add("pf-default-pick", PREC_F32, "streams", 17, 84, 64, pad=(3, 0, 64), opts={"prefill_attn": -1})
    return cases


CASES = _build()


# ---------------------------------------------------------------------------------------------------------------------------------------
# geometry: who reads what
# ---------------------------------------------------------------------------------------------------------------------------------------
def row_maps(nseq, Tmax):
    """The two row maps [nseq][Tmax]: rows 0 .. 5, different for every sequence at a position, and never equal to each other."""
    t = torch.arange(Tmax)[None, :]
    b = torch.arange(nseq)[:, None]
    m0 = (2 * b + (t * 5 + 1) // 3) % MAP_ROWS
    m1 = (m0 + 1 + 2 * (t % 2)) % MAP_ROWS
    return m0, m1


class Geo:
    pass


def geometry(c, mutant=None):
    """first / last / physical row of every (sequence, query, key) of the case.  mutant: one deliberate defect (MUTANTS); returns None when the
    defect changes nothing in this case."""
    g = Geo()
    nq, T = c.nq, c.Tmax
    b = torch.arange(c.nseq)
    g.pb = torch.tensor(c.seq_map) if (c.seq_map is not None and mutant != "no_seq_map") else b * max(c.seq_mul, 1)
    if mutant == "no_seq_map":
        g.pb = g.pb % ROWS                                                           # (the 130-sequence launch: stay inside the tables)
    pad = torch.tensor(c.pad) if c.pad is not None else torch.zeros(ROWS, dtype=torch.long)
    shift = torch.tensor(c.shift) if (c.shift is not None and mutant != "no_pos_shift") else torch.zeros(ROWS, dtype=torch.long)
    g.first = pad[g.pb]
    g.last = (c.pos + torch.arange(nq)[None, :] - shift[g.pb][:, None]).clamp(max=T - 1)
    if c.rmap:
        m0, m1 = row_maps(c.nseq, T)
        g.rows = (m1, m0)[(c.step & 1) ^ (mutant != "parity")]
    else:
        g.rows = g.pb[:, None].expand(c.nseq, T)
    lo, hi = g.first[:, None].expand(c.nseq, nq), g.last
    if mutant == "first-1":
        lo = (lo - 1).clamp(min=0)
    elif mutant == "first+1":
        lo = lo + 1
    elif mutant == "last+1":
        hi = (hi + 1).clamp(max=T - 1)
    elif mutant == "last-1":
        hi = hi - 1
    t = torch.arange(T)
    g.mask = (t >= lo[:, :, None]) & (t <= hi[:, :, None])                         # [nseq][nq][T]
    if mutant and mutant.startswith("drop@first+"):
        p = g.first + int(mutant.split("+")[1])
        interior = (p[:, None] > lo) & (p[:, None] < hi)                           # a key strictly inside the query's window
        g.mask = g.mask & ~(interior[:, :, None] & (t == p[:, None, None]))
    g.kvhead = torch.tensor([1, 0] if mutant == "heads" else [0, 1])
    if mutant:
        if c.rmap is False and mutant == "parity":
            return None
        ref = geometry(c)
        used = ref.mask.any(1) | g.mask.any(1)
        if torch.equal(ref.mask, g.mask) and torch.equal(ref.rows[used], g.rows[used]) and torch.equal(ref.kvhead, g.kvhead):
            return None
    return g


def attend(q, k, v, g, dtype=torch.float64, parts=None):
    """The definition, evaluated densely in `dtype`: returns (out [nseq][nq][D], sum_t w_t |v_td| [nseq][nq][D]).
    q [nseq][nq][D]; k, v [ROWS][H][Tmax][64].  parts: a dict that receives the weights and the gathered K / V (for hilo_term)."""
    nseq, nq, T = g.mask.shape
    t = torch.arange(T)
    kg = k[g.rows[:, None, :], g.kvhead[None, :, None], t[None, None, :]].to(dtype)      # [nseq][H][T][64]: the row that holds key t of sequence b
    vg = v[g.rows[:, None, :], g.kvhead[None, :, None], t[None, None, :]].to(dtype)
    used = g.mask.any(1)                                                                 # keys some query of the sequence sees
    vg = torch.where(used[:, None, :, None], vg, torch.zeros((), dtype=dtype))
    s = torch.einsum("bqhd,bhtd->bhqt", q.view(nseq, nq, H, HD).to(dtype), kg) / 8
    m = g.mask[:, None, :, :]
    w = torch.softmax(torch.where(m, s, torch.full((), -math.inf, dtype=dtype)), dim=-1)
    w = torch.where(m.any(-1, keepdim=True), w, torch.zeros((), dtype=dtype))            # an empty window: 0
    out = torch.einsum("bhqt,bhtd->bqhd", w, vg).reshape(nseq, nq, D)
    absw = torch.einsum("bhqt,bhtd->bqhd", w, vg.abs()).reshape(nseq, nq, D)
    if parts is not None:
        parts.update(w=w, kg=kg, vg=vg)
    return out, absw


def hilo_term(q, g, ref, absw, parts):
    """What the bf16 MFMA kernel's operand format costs, first order, elementwise.  attn_prefill_mfma_kernel<true> feeds the matrix pipe bf16
    operands: the f32 query (times 1/8, exact) and the probabilities p_t = exp(s_t - m) are each carried as a pair hi = bf16(x), lo = bf16(x - hi)
    (gpt_kernels.hip: "16 significant bits").  Both conversions round to nearest: |x - hi| <= 2^-9 |x|, |x - hi - lo| <= 2^-9 |x - hi|, so
    every query component and every probability enters its MFMA with a relative error of at most d = 2^-18.
      probabilities: the numerator sums p_t (1 + e_t) v_td, |e_t| <= d, while the denominator sums the f32 p_t: an error of at most
        d sum_t w_t |v_td|.
      query: the score of key t moves by at most ds_t = d A_t, A_t = sum_j |q_j| |k_tj| / 8; the weights become w_t exp(ds_t) / sum_u w_u exp(ds_u),
        and to first order the output moves by sum_t w_t ds_t (v_td - out_d): at most d (sum_t w_t A_t |v_td| + |out_d| sum_t w_t A_t).
    (d A_t is about 1e-4 for the random family's operands, so the second order is some 1e-8 of the same sums.)  The stream kernel and the f32 MFMA
    kernel work on f32 operands and get no such term.  On the MI355X the 4 E limit alone was exceeded by up to 1.48 x in four bf16 MFMA cases;
    evaluating the reference with the query alone carried as hi + lo reproduces 1.32 x of it, the probabilities alone 0.13 x, the argument
    rounding of __expf 0.01 x."""
    d = 2.0 ** -18
    nseq, nq, _ = ref.shape
    A = torch.einsum("bqhd,bhtd->bhqt", q.view(nseq, nq, H, HD).double().abs(), torch.nan_to_num(parts["kg"].abs(), nan=0.0)) / 8
    wA = parts["w"] * torch.where(g.mask[:, None, :, :], A, torch.zeros((), dtype=torch.float64))
    t1 = torch.einsum("bhqt,bhtd->bqhd", wA, parts["vg"].abs()).reshape(nseq, nq, D)
    t2 = ref.abs() * wA.sum(-1).permute(0, 2, 1)[:, :, :, None].expand(nseq, nq, H, HD).reshape(nseq, nq, D)
    return d * (absw + t1 + t2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------------------------
def _gen(c, salt):
    return torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()) * 8 + salt)


@functools.lru_cache(maxsize=4)
def cells(c):
    """(visible, finite) [ROWS][Tmax]: cells some query of the launch sees; cells inside what the launch's tables name (a named row up to the last
    key written for a sequence that names it).  finite & ~visible is poisoned, ~finite holds NaN."""
    g = geometry(c)
    used = g.mask.any(1)
    tt = torch.arange(c.Tmax)[None, :].expand(c.nseq, c.Tmax)
    visible = torch.zeros(ROWS, c.Tmax, dtype=torch.bool)
    visible[g.rows[used], tt[used]] = True
    hi = torch.full((ROWS,), -1, dtype=torch.long)
    for b in range(c.nseq):
        named = set(g.rows[b][used[b]].tolist()) | {int(g.pb[b])}
        for r in named:
            hi[r] = max(int(hi[r]), int(g.last[b, -1]))
    finite = torch.arange(c.Tmax)[None, :] <= hi[:, None]
    assert bool((visible <= finite).all())
    return visible, finite


def _fill(c, vis_vals, poison_val):
    """[ROWS][H][Tmax][64] f32: vis_vals where visible, the poison value in the other finite cells, NaN elsewhere."""
    visible, finite = cells(c)
    x = torch.full((ROWS, H, c.Tmax, HD), NAN)
    x = torch.where(finite[:, None, :, None], poison_val if torch.is_tensor(poison_val) else torch.full((), float(poison_val)), x)
    return torch.where(visible[:, None, :, None], vis_vals, x)


def _engine_values(x, prec):
    return x.bfloat16().float() if prec == PREC_BF16 else x


OneHot = collections.namedtuple("OneHot", "rule q idx val expect")          # K patch: k[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]] = val


@functools.lru_cache(maxsize=2)
def onehot_operands(c):
    """(k0, v, launches): the K image before a launch's patch, V, and per launch the query, the K patch and the expected output."""
    gen = _gen(c, 1)
    shape = (ROWS, H, c.Tmax, HD)
    mag = torch.randint(1, 256, shape, generator=gen).float() * (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1)
    k0 = _fill(c, torch.zeros(()), K_POISON)
    v = _engine_values(_fill(c, mag, POISON_V), c.prec)
    g = geometry(c)
    first, last, rows = g.first.tolist(), g.last.tolist(), g.rows
    launches = []
    for rule in ONEHOT_RULES:
        # the target of every query, where the rule has one inside its window
        plan, applies = {}, False          # (b, h) -> list over launches of {position: slot}; query -> (launch, position)
        target = {}
        for b in range(c.nseq):
            for qi in range(c.nq):
                f, l = first[b], last[b][qi]
                if l < f:
                    continue
                tq = {"first": f, "last": l, "last-1": l - 1}.get(rule)
                if tq is None:
                    tq = f + int(rule.split("+")[1])
                if tq < f or tq > l:
                    tq = f
                applies |= tq != f or rule == "first"
                passes = plan.setdefault(b, [{}])
                if tq != f and tq not in passes[-1]:
                    if len(passes[-1]) == SLOTS:
                        passes.append({})
                    passes[-1][tq] = len(passes[-1])
                target[b, qi] = (len(passes) - 1, tq)
        if not applies:
            continue
        for p in range(max(len(x) for x in plan.values()) if plan else 1):
            q = torch.zeros(c.nseq, c.nq, D)
            expect = torch.zeros(c.nseq, c.nq, D)
            idx, val = [], []
            for (b, qi), (pq, tq) in target.items():
                f = first[b]
                own = pq == p and tq != f
                tpos = tq if own else f
                for h in range(H):
                    dim = ((plan[b][p][tq] if own else SLOTS) + 5 * h + 3 * int(g.pb[b])) % HD
                    q[b, qi, h * HD + dim] = Q_HOT
                    r = int(rows[b, tpos])
                    idx.append((r, h, tpos, dim)); val.append(K_HOT)
                    expect[b, qi, h * HD:(h + 1) * HD] = v[r, h, tpos]
                    if own and rule == "last" and tq + 1 <= last[b][-1]:                  # the next query's key must not be seen by this one
                        idx.append((int(rows[b, tq + 1]), h, tq + 1, dim)); val.append(K_POISON)
            launches.append(OneHot(f"{rule}#{p}", q, torch.tensor(idx, dtype=torch.long).reshape(-1, 4), torch.tensor(val), expect))
    return k0, v, launches


def patched(k0, oh):
    k = k0.clone()
    if oh.idx.numel():
        i = oh.idx.to(k0.device)
        k[i[:, 0], i[:, 1], i[:, 2], i[:, 3]] = oh.val.to(k0.device, k0.dtype)
    return k


@functools.lru_cache(maxsize=2)
def uniform_operands(c):
    """(q = 0, k, v): small-integer keys (their score is 0 whatever they hold), V integers in 1 .. 255."""
    gen = _gen(c, 2)
    shape = (ROWS, H, c.Tmax, HD)
    k = _fill(c, torch.randint(-3, 4, shape, generator=gen).float(), K_POISON)
    v = _engine_values(_fill(c, torch.randint(1, 256, shape, generator=gen).float(), POISON_V), c.prec)
    return torch.zeros(c.nseq, c.nq, D), k, v


@functools.lru_cache(maxsize=2)
def random_operands(c):
    """(q, k, v): scores q . k / 8 of standard deviation 2.5 (about +-8 over a thousand keys); |v| log-normal (sigma 1.5), either sign.  A key that
    must not be seen is an ordinary key (an ordinary weight) with V = 1e30."""
    gen = _gen(c, 3)
    shape = (ROWS, H, c.Tmax, HD)
    q = torch.randn(c.nseq, c.nq, D, generator=gen) * 2.5
    kr = torch.randn(shape, generator=gen)
    k = _engine_values(_fill(c, kr, kr), c.prec)
    v = _engine_values(_fill(c, torch.randn(shape, generator=gen) * torch.exp(1.5 * torch.randn(shape, generator=gen)), POISON_V), c.prec)
    return q, k, v


def to_engine(x, prec):
    """What the engine's output dtype makes of exact values (the host test's mutants go through the same rounding)."""
    x = x.float()
    return x.bfloat16() if prec == PREC_BF16 else x


# ---------------------------------------------------------------------------------------------------------------------------------------
# the comparisons (an empty list = the output passes)
# ---------------------------------------------------------------------------------------------------------------------------------------
def bf16_step(x):
    """One step of the bf16 grid at |x| (8 significant bits): 2^(floor(log2 |x|) - 7); 0 at 0."""
    _, e = torch.frexp(x.double().abs())
    return torch.where(x == 0, torch.zeros((), dtype=torch.float64), torch.ldexp(torch.ones((), dtype=torch.float64), e - 8))


def f32_ulp(x):
    _, e = torch.frexp(x.double().abs())
    return torch.where(x == 0, torch.zeros((), dtype=torch.float64), torch.ldexp(torch.ones((), dtype=torch.float64), e - 24))


def check_canary(out):
    """out: the output block in the engine's dtype.  No NaN (an element never written keeps its NaN pre-fill; a NaN cell was read) and no Inf."""
    bad = ~torch.isfinite(out.float())
    return [f"{int(bad.sum())} of {out.numel()} output elements are NaN / Inf; first at {bad.nonzero()[0].tolist()}"] if bool(bad.any()) else []


def check_onehot(out, expect, prec):
    want = to_engine(expect, prec)
    same = out.view(torch.int16 if prec == PREC_BF16 else torch.int32) == want.view(torch.int16 if prec == PREC_BF16 else torch.int32)
    if bool(same.all()):
        return []
    bad = (~same).nonzero()
    i = tuple(bad[0].tolist())
    return [f"{bad.shape[0]} of {out.numel()} elements differ from the target's V row; first at (seq, query, dim) {list(i)}: {float(out[i])} vs "
            f"{float(want[i])}; sequences {sorted(set(bad[:, 0].tolist()))[:8]} queries {sorted(set(bad[:, 1].tolist()))[:8]}"]


def check_uniform(out, ref, prec):
    tol = bf16_step(ref) if prec == PREC_BF16 else 2 * f32_ulp(ref)
    err = (out.double() - ref).abs()
    bad = ~(err <= tol)
    if not bool(bad.any()):
        return []
    i = tuple(bad.nonzero()[0].tolist())
    return [f"{int(bad.sum())} of {out.numel()} means are off; first at {list(i)}: {float(out[i])} vs {float(ref[i])} (a count of keys off by one "
            f"moves the mean by 1 / n)"]


def random_limit(c, q, k, v):
    """(ref, limit, E): the f64 result, the elementwise limit and the plain-f32 figure it is built on."""
    g = geometry(c)
    parts = {}
    ref, absw = attend(q, k, v, g, parts=parts)
    f32, _ = attend(q, k, v, g, torch.float32)
    err = (f32.double() - ref).abs()
    E = float(torch.where(absw > 0, err / absw, torch.zeros((), dtype=torch.float64)).max())
    limit = 4 * E * absw
    if c.prec == PREC_BF16:
        limit = limit + bf16_step(ref)
        if c.kind == "mfma":
            limit = limit + hilo_term(q, g, ref, absw, parts)
    return ref, limit, E


def random_ratio(out, ref, limit):
    """Largest error / limit (inf where the limit is 0 and the output is not the reference: an empty window gives 0 exactly)."""
    err = (out.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros((), dtype=torch.float64), err / limit)
    return float(torch.nan_to_num(r, nan=math.inf).max())


def check_random(out, ref, limit):
    r = random_ratio(out, ref, limit)
    return [f"largest error / limit = {r:.3f}"] if not r <= 1.0 else []


Launch = collections.namedtuple("Launch", "label q k v check ratio")


def launches(c):
    """Every launch of the case: operands, check(out [nseq][nq][D] in the engine's dtype) -> list of failures, and for the random family
    ratio(out) -> largest error / limit."""
    k0, v, hots = onehot_operands(c)
    for oh in hots:
        yield Launch("onehot " + oh.rule, oh.q, patched(k0, oh), v, lambda out, oh=oh: check_canary(out) + check_onehot(out, oh.expect, c.prec), None)
    q, k, v = uniform_operands(c)
    uref, _ = attend(q, k, v, geometry(c))
    yield Launch("uniform", q, k, v, lambda out: check_canary(out) + check_uniform(out, uref, c.prec), None)
    q, k, v = random_operands(c)
    ref, limit, _ = random_limit(c, q, k, v)
    yield Launch("random", q, k, v, lambda out: check_canary(out) + check_random(out, ref, limit), lambda out: random_ratio(out, ref, limit))
