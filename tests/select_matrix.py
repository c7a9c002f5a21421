"""The token-selection test matrix shared by tests/test_gpu_select_matrix.py (GPU) and tests/test_select_matrix_host.py (CPU): crafted score
rows in front of `sample_kernel`, `beam_rows_kernel`, `beam_step_kernel` and `beam_apply_kernel` (csrc/gpt_kernels.hip), the settings and
uniform streams each row is decoded with, and the ids it must give.  No GPU import.

How a row reaches the kernels.  A "constant-logits model": the tiny fixture's geometry (3 layers, model dim 128, 2 heads,
`gpt_oracle.synth_weights`) with `mel_head.weight = 0` and `mel_head.bias = row`.  The head GEMM then adds the bias to a sum of exact zeros:
the logits ARE the row at every step, in every batch row, in the fp32 and in the bf16 engine (a -0.0 in the row arrives as +0.0, in the
oracle too).  A step changes only the seen set, the row's own step and the beam state.  The vocabulary size is a parameter of both
`GPTConfig` and `gpt.UnifiedVoice` (start = V - 2, stop = V - 1 here).

Expected ids: `oracle.gpt_oracle` in f32 on the same weights under `GenParams(tie_rule="index")` -- the engine's rule for exact ties, which
the reference leaves to whatever torch.sort / torch.topk do (DESIGN: "Token selection: ties, caps, the top-p threshold").  Two kinds of case
cannot take them from the oracle, and say so in their fields:
  * `cap`: more scores tie on the k-th value than the kernel has survivor slots.  The rule (every score strictly above the threshold, then
    the tied ones of lowest index up to the cap) is the engine's own; the ids come from the restatement below with that cap.
  * `engine_thr`: the one case that sits on the 1-ulp difference between the reference's top-p threshold (f32 of `1 - top_p` formed in
    double) and the engine's (`1 - top_p` formed from the f32 `top_p`); the ids are the restatement's under the engine's threshold, and the
    host file shows what the reference gives.

The restatement (`run_rows`, `run_beam`): the selection written out plainly on one score row, with no transformer around it, in f32 or f64.
tests/test_select_matrix_host.py holds it to the oracle's ids on every case, uses its f64 run as the high-precision reference of the margin
gate (the oracle casts its logits to f32), and flips one named defect at a time (`DEFECTS`) to show that the table notices each.

Row values are quarter-integers over a floor of -64, penalties and temperatures powers of two: f32 and f64 process them to the same values.
The selection kernels' paths by vocabulary size: 200 (fewer scores than the 256 threads), 257 (one thread holds two), 8194 (production,
32 * 256 + 2), 8448 (256 * TOPK_KPT, the last size of the ballot bisection), 8449 (the first that falls to the radix select unasked; with
typical sampling 67.6 KB of dynamic LDS).  `radix` lists the `sample_radix` option values a case runs at (None: the kernel's default)."""
import collections
import functools
import math

import torch

from oracle import gpt_oracle as G

GEOM = dict(layers=3, model_dim=128, heads=2, max_text_tokens=20, max_mel_tokens=30, number_text_tokens=60)
WEIGHT_SEED = 1234
SIZES = (200, 257, 8194, 8448, 8449)
SAMPLE_CAP, BEAM_CAP = 128, 64               # survivor slots of sample_kernel / beam_rows_kernel (gpt_kernels.hip)
FLOOR = -64.0
NINF = float("-inf")
U_LAST = 1.0 - 2.0 ** -53
SCORE_MARGIN, CDF_MARGIN = 1e-4, 1e-9        # the margin gate: scores and cumulative probabilities / u * total against the CDF steps

Case = collections.namedtuple("Case", "name family V row B max_new st rows uniforms row_max_new radix ties cap engine_thr gate walk why")
# family: "greedy" | "sample" | "beam";  row: (V,) f32;  st: the call's scalar settings (generate kwargs);  rows: per-row (`row_sampling`) or
# per-utterance (`group_sampling`) dicts over st, or None;  uniforms: (max_new, B) f64, beams (max_new, B, 2 nb), or None;
# ties: the ids depend on the tie rule;  gate: the margin gate applies;  walk: the ids the draws must cover between them, or None


def config(V: int) -> G.GPTConfig:
    return G.GPTConfig(number_mel_codes=V, start_mel_token=V - 2, stop_mel_token=V - 1, **GEOM)


def weights(V: int, row: torch.Tensor) -> dict:
    sd = G.synth_weights(config(V), seed=WEIGHT_SEED)
    sd["mel_head.weight"] = torch.zeros_like(sd["mel_head.weight"])
    sd["mel_head.bias"] = row.clone().float()
    return sd


def inputs(B: int):
    """-> text (B, 6), langs (B,), style (1, 192), emo (1, D): the same for every case; the logits do not depend on them"""
    g = torch.Generator().manual_seed(5)
    text = torch.randint(2, GEOM["number_text_tokens"], (4, 6), generator=g)
    text[1, 4:] = 1
    style = torch.randn(1, 192, generator=g)
    emo = torch.randn(1, GEOM["model_dim"], generator=g) * 0.1
    return text[:B].contiguous(), torch.tensor([1, 2, 3, 1])[:B].contiguous(), style, emo


def make_row(V: int, values: dict, floor: float = FLOOR) -> torch.Tensor:
    r = torch.full((V,), floor, dtype=torch.float32)
    for i, v in values.items():
        assert 0 <= i < V, (i, V)
        r[i] = v
    return r


def gen_params(case: Case, st: dict, max_new: int, tie_rule="index") -> G.GenParams:
    nb = int(st.get("num_beams", 1))
    return G.GenParams(do_sample=bool(st.get("do_sample", False)), num_beams=nb, top_p=float(st.get("top_p", 1.0)), top_k=int(st.get("top_k", 50)),
                       temperature=float(st.get("temperature", 1.0)), repetition_penalty=float(st.get("repetition_penalty", 1.0)),
                       length_penalty=float(st.get("length_penalty", 1.0)), typical_sampling=float(st.get("typical_mass", 0.0)) > 0.0,
                       typical_mass=float(st.get("typical_mass", 0.0)) or 0.9, max_generate_length=int(max_new), tie_rule=tie_rule,
                       min_tokens_to_keep=st.get("min_tokens_to_keep"))


def unit_settings(case: Case):
    """the settings of every row (beams: utterance) of the case: the scalars, overlaid by its own table entry"""
    return [dict(case.st, **(case.rows[b] if case.rows is not None else {})) for b in range(case.B)]


def unit_caps(case: Case):
    return [case.max_new if case.row_max_new is None else min(case.max_new, int(case.row_max_new[b])) for b in range(case.B)]


def assemble(unit_ids, stop: int, max_new: int, cut: bool = True) -> torch.Tensor:
    """rows of ragged ids -> what a call returns: as wide as the longest row up to and including its first stop token, stop tokens behind
    (cut=False: whatever the row holds behind its first stop token stays)"""
    rows, ends = [], []
    for ids in unit_ids:
        ids = [int(t) for t in ids]
        ends.append(ids.index(stop) + 1 if stop in ids else len(ids))
        rows.append(ids[: ends[-1]] if cut else ids)
    n = min(max(ends), max_new)
    return torch.tensor([(r + [stop] * n)[:n] for r in rows], dtype=torch.int64)


# ----------------------------------------------------------------------------------------------------------------
# the oracle's ids
# ----------------------------------------------------------------------------------------------------------------
def oracle_ids(case: Case, tie_rule="index", trace=None) -> torch.Tensor:
    """`gpt_oracle.inference_speech` in f32 on the case's weights, one run per row (utterance) with that unit's own settings, cap and column of
    the uniform stream -- rows of a batch do not interact -- assembled as one call returns them."""
    cfg = config(case.V)
    sd = weights(case.V, case.row)
    text, langs, style, emo = inputs(case.B)
    conds = G.conds_latent_campplus(sd, style, emo)
    out = []
    for b, (st, cap) in enumerate(zip(unit_settings(case), unit_caps(case))):
        u = None if case.uniforms is None else case.uniforms[:, b:b + 1]
        tr = {} if trace is not None else None
        with torch.no_grad():
            ids = G.inference_speech(sd, cfg, conds, text[b:b + 1], langs[b:b + 1], gen_params(case, st, cap, tie_rule), u, True, tr)
        if trace is not None:
            trace.append(tr)
        out.append(ids[0].tolist() + [cfg.stop_mel_token])          # (a row stopped by its cap emits the stop token from there on)
    return assemble(out, cfg.stop_mel_token, case.max_new)


# ----------------------------------------------------------------------------------------------------------------
# the restatement
# ----------------------------------------------------------------------------------------------------------------
DEFECTS = (
    "top-p: < for <=",
    "ties to the higher index",
    "penalty divides negative scores",
    "fake-prompt ids unseen",
    "temperature before typical",
    "min_keep ignored",
    "inverse CDF: >= for >",
    "k off by one",
    "no forced stop after the first stop token",
    "stop candidate of rank >= nb added",
    "length penalty ignored",
    "worst not updated on replacement",
    "done rule: > for >=",
)


class Log:
    """what a restatement run decided on: `margins[kind]` = |a - b| of every comparison (kind: "score" | "cum" | "cdf"), `events` = names of
    the beam scorer's branches taken"""

    def __init__(self):
        self.margins = {"score": [], "cum": [], "cdf": []}
        self.events = set()

    def cmp(self, kind: str, a, b):
        self.margins[kind].append(abs(float(a) - float(b)))

    def near(self):
        """the comparisons that are neither exact ties nor decided by the gate's margin"""
        bound = {"score": SCORE_MARGIN, "cum": SCORE_MARGIN, "cdf": CDF_MARGIN}
        return [(k, m) for k, ms in self.margins.items() for m in ms if 0.0 < m < bound[k]]


def _gap_below(x: torch.Tensor, v: float):
    """the largest value of x strictly below v (None: there is none)"""
    lower = x[x < v]
    return float(lower.max()) if lower.numel() else None


def _penalise(x, seen, pen: float, defect):
    if pen == 1.0 or not seen:
        return x
    ids = torch.tensor(sorted(seen))
    s = x[ids]
    x = x.clone()
    x[ids] = s / pen if defect == "penalty divides negative scores" else torch.where(s < 0, s * pen, s / pen)
    return x


def _typical(x, mass: float, min_keep: int, log):
    """indextts/utils/typical_sampling.py: keep the tokens whose |-log p - H| is at most that of the token on which the mass, accumulated in
    ascending order of that distance, reaches `mass`"""
    nl = torch.log_softmax(x, dim=-1)
    p = torch.exp(nl)
    ent = -(nl * p).nansum()
    s = torch.abs((-nl) - ent)
    ss, order = torch.sort(s, stable=True)
    cum = torch.softmax(x[order], dim=-1).cumsum(-1)
    last = min(int((cum < mass).sum()), x.numel() - 1)
    thr = ss[last]
    remove = s > thr
    if min_keep > 1:
        remove[order[:min_keep]] = False
    if log is not None:                                      # by value groups: the mass before the threshold's group and behind it
        before = cum[int((ss < thr).sum()) - 1] if bool((ss < thr).any()) else 0.0
        log.cmp("cum", before, mass)
        log.cmp("cum", cum[int((ss <= thr).sum()) - 1], mass)
        for other in (ss[ss < thr][-1:].tolist() + ss[ss > thr][:1].tolist()):
            if math.isfinite(other):
                log.cmp("score", other, thr)
    return x.masked_fill(remove, NINF)


def _processed(row, seen, st, dtype, defect, log, min_keep):
    """the score processors up to (not including) top-k: repetition penalty, typical filter, temperature"""
    x = _penalise(row.to(dtype), seen, float(st.get("repetition_penalty", 1.0)), defect)
    T = float(st.get("temperature", 1.0))
    temp = bool(st.get("do_sample", False)) and T != 1.0
    mass = float(st.get("typical_mass", 0.0))
    if mass > 0.0:
        early = defect == "temperature before typical"
        if temp and early:
            x = x / T
        x = _typical(x, mass, min_keep, log)
        if temp and not early:
            x = x / T
    elif temp:
        x = x / T
    return x


def _at_least(x, kth: float, cap):
    """the indices of the finite scores >= kth; more of them than `cap` slots: those above kth, then the tied ones of lowest index"""
    ids = torch.nonzero((x >= kth) & (x > NINF)).flatten()
    if cap is not None and ids.numel() > cap:
        above, tied = ids[x[ids] > kth], ids[x[ids] == kth]
        ids = torch.sort(torch.cat([above, tied[: cap - above.numel()]]))[0]
    return ids


def _survivors(x, st, dtype, defect, log, min_keep, cap, engine_thr):
    """top-k and top-p of one processed row -> (ids, scores) of the kept set, ascending by (score, index)"""
    V = x.numel()
    k = min(max(int(st.get("top_k", 50)), min_keep), V)
    if defect == "k off by one":
        k = max(k - 1, 1)
    kth = float(torch.sort(x, descending=True)[0][k - 1])
    below = _gap_below(x, kth)
    if log is not None and below is not None and math.isfinite(below):
        log.cmp("score", kth, below)
    ids = _at_least(x, kth, cap)
    if defect == "ties to the higher index":
        ids = ids.flip(0)
    v, order = torch.sort(x[ids], stable=True)
    ids = ids[order]
    n = ids.numel()
    lo = 0
    top_p = float(st.get("top_p", 1.0))
    if top_p < 1.0:
        cum = torch.softmax(v, dim=-1).cumsum(-1)
        if engine_thr:                                       # gpt_kernels.hip: (float)(1.0 - (double)top_p) of the f32 top_p
            thr = torch.tensor(1.0 - float(torch.tensor(top_p, dtype=torch.float32)), dtype=torch.float32).to(dtype)
        else:                                                # the reference: `cum <= (1 - top_p)`, the double rounded once to the tensor's type
            thr = torch.tensor(1.0 - top_p, dtype=dtype)
        keep = 0 if defect == "min_keep ignored" else max(min_keep, 1)
        for i in range(min(n - keep, n - 1)):
            if log is not None:
                log.cmp("cum", cum[i], thr)
            if (cum[i] < thr) if defect == "top-p: < for <=" else (cum[i] <= thr):
                lo = i + 1
            else:
                break
    return ids[lo:], v[lo:]


def _draw(p64, u: float, defect, log):
    """index of the first entry whose running f64 sum exceeds u * total (the last live entry when none does)"""
    c = p64.cumsum(0)
    tgt = u * float(c[-1])
    if log is not None:                                      # (the last step IS the total, and past it the pick falls back to the last live entry)
        inner = c[c < c[-1]]
        if inner.numel():
            log.cmp("cdf", float((inner - tgt).abs().min()), 0.0)
    hit = (c >= tgt) if defect == "inverse CDF: >= for >" else (c > tgt)
    hit = hit & (p64 > 0)
    live = torch.nonzero(p64 > 0).flatten()
    return int(torch.nonzero(hit).flatten()[0]) if bool(hit.any()) else int(live[-1])


def _select(row, seen, st, u, dtype, defect, log, cap, engine_thr):
    """one step of one row -> (token, log-probability of the token under the distribution it was selected with, in `dtype`)"""
    min_keep = int(st.get("min_tokens_to_keep") or 1)
    x = _processed(row, seen, st, dtype, defect, log, min_keep)
    if not st.get("do_sample", False):
        m = float(x.max())
        idx = torch.nonzero(x == m).flatten()
        below = _gap_below(x, m)
        if log is not None and below is not None and math.isfinite(below):
            log.cmp("score", m, below)
        tok = int(idx[-1] if defect == "ties to the higher index" else idx[0])
        return tok, float(torch.log_softmax(x.double(), -1)[tok])
    ids, v = _survivors(x, st, dtype, defect, log, min_keep, cap, engine_thr)
    ids, order = torch.sort(ids)                             # the kept set in vocabulary order
    p = torch.softmax(v[order], dim=-1)
    at = _draw(p.double(), float(u), defect, log)
    return int(ids[at]), float(torch.log(p.double()[at] / p.double().sum()))


def run_rows(case: Case, dtype=torch.float32, defect=None, log=None, scores=None) -> torch.Tensor:
    """greedy / sampling cases -> the ids of the call.  scores: a list that receives, per row, [(logp_model, logp_sampled) per stored token the
    selection chose itself] in f64 arithmetic on the `dtype` values."""
    V, stop, start = case.V, case.V - 1, case.V - 2
    logp_raw = torch.log_softmax(case.row.double(), -1)
    out = []
    for b, (st, cap) in enumerate(zip(unit_settings(case), unit_caps(case))):
        seen = set() if defect == "fake-prompt ids unseen" else {1, start}
        ids, sc, finished = [], [], False
        for step in range(case.max_new):
            forced = (finished and defect != "no forced stop after the first stop token") or step >= cap
            if forced:
                tok = stop
            else:
                u = None if case.uniforms is None else float(case.uniforms[step, b])
                tok, lsel = _select(case.row, seen, st, u, dtype, defect, log, SAMPLE_CAP if case.cap else None, case.engine_thr)
                if not finished:
                    sc.append((float(logp_raw[tok]), lsel))
            ids.append(tok)
            seen.add(tok)
            finished = finished or tok == stop
        out.append(ids)
        if scores is not None:
            scores.append(sc)
    return assemble(out, stop, case.max_new, cut=defect != "no forced stop after the first stop token")


class _Hyps:
    """BeamHypotheses (transformers_beam_search.py:930-1013), early_stopping=False"""

    def __init__(self, nb, lp, defect, log):
        self.nb, self.lp, self.defect, self.log = nb, lp, defect, log
        self.beams, self.worst = [], 1e9

    def add(self, seq, sum_logprobs: float, gen_len: int):
        score = sum_logprobs if self.defect == "length penalty ignored" else sum_logprobs / (gen_len ** self.lp)
        if len(self.beams) >= self.nb:
            self.log.cmp("score", score, self.worst)
        if len(self.beams) < self.nb or score > self.worst:
            self.beams.append((score, list(seq)))
            if len(self.beams) > self.nb:
                order = sorted((s, i) for i, (s, _) in enumerate(self.beams))
                del self.beams[order[0][1]]
                self.log.events.add("a better hypothesis replaced the worst")
                if self.defect != "worst not updated on replacement":
                    self.worst = order[1][0]
            else:
                self.worst = min(score, self.worst)
                if len(self.beams) == self.nb:
                    self.log.events.add("the heap filled")
        elif len(self.beams) >= self.nb:
            self.log.events.add("a hypothesis no better than the worst was dropped")

    def is_done(self, best_sum: float, gen_len: int) -> bool:
        if len(self.beams) < self.nb:
            return False
        highest = best_sum / gen_len ** self.lp
        self.log.cmp("score", self.worst, highest)
        fired = self.worst > highest if self.defect == "done rule: > for >=" else self.worst >= highest
        self.log.events.add("the done rule fired" if fired else "the done rule did not fire on a full heap")
        return fired


def jittered(row: torch.Tensor, logp: torch.Tensor, seed: int) -> torch.Tensor:
    """log-probabilities another correct f32 log_softmax could give: every distinct row value's result moved by -1, 0 or +1 ulp (equal scores
    stay equal: they go through the same arithmetic)"""
    vals, inv = torch.unique(row, return_inverse=True)
    shift = torch.randint(-1, 2, (vals.numel(),), generator=torch.Generator().manual_seed(seed))[inv]
    up, down = torch.nextafter(logp, torch.full_like(logp, math.inf)), torch.nextafter(logp, torch.full_like(logp, -math.inf))
    return torch.where(shift > 0, up, torch.where(shift < 0, down, logp))


def _beam_unit(case: Case, st, us, dtype, defect, log, jitter=None):
    V, stop, start = case.V, case.V - 1, case.V - 2
    nb, lp, sample = int(st["num_beams"]), float(st.get("length_penalty", 1.0)), bool(st.get("do_sample", False))
    min_keep = int(st.get("min_tokens_to_keep") or 2)
    logp = torch.log_softmax(case.row.to(dtype), -1)
    if jitter is not None:
        logp = jittered(case.row, logp, jitter)
    seqs = [[] for _ in range(nb)]
    seens = [set() if defect == "fake-prompt ids unseen" else {1, start} for _ in range(nb)]
    scores = torch.tensor([0.0] + [-1e9] * (nb - 1), dtype=dtype)
    hyps, done = _Hyps(nb, lp, defect, log), False
    for step in range(case.max_new):
        flat, val = [], []
        for j in range(nb):
            x = _processed(logp, seens[j], st, dtype, defect, log, min_keep)
            if sample:
                ids, v = _survivors(x, st, dtype, defect, log, min_keep, BEAM_CAP if case.cap else None, case.engine_thr)
                ids, order = torch.sort(ids)
                v = v[order]
            elif case.cap:                                   # beam search keeps the row's top 2 nb, ties included, in BEAM_CAP slots
                ids = _at_least(x, float(torch.sort(x, descending=True)[0][min(2 * nb, V) - 1]), BEAM_CAP)
                v = x[ids]
            else:
                ids, v = torch.arange(V), x
            flat.append(ids + j * V)
            val.append(v + scores[j])
        flat, val = torch.cat(flat), torch.cat(val)
        if sample:
            p = torch.softmax(val, -1).double()
            picks = []
            for d in range(2 * nb):
                at = _draw(p, float(us[step, d]), defect, log)
                picks.append(at)
                p[at] = 0.0
            picks = torch.tensor(picks)
            order = torch.sort(val[picks], descending=True, stable=True)[1]
            cand = picks[order]
        else:
            if defect == "ties to the higher index":
                cand = (val.numel() - 1 - torch.sort(val.flip(0), descending=True, stable=True)[1])[: 2 * nb + 1]
            else:
                cand = torch.sort(val, descending=True, stable=True)[1][: 2 * nb + 1]
            for a, b2 in zip(cand[:-1], cand[1:]):           # every rank boundary down to the first candidate left out
                if math.isfinite(float(val[b2])):
                    log.cmp("score", val[a], val[b2])
            cand = cand[: 2 * nb]
        gen_len, new = step + 1, []
        for rank, c in enumerate(cand.tolist()):
            tok, src, sc = int(flat[c]) % V, int(flat[c]) // V, val[c]
            if tok == stop:
                if rank >= nb:
                    log.events.add("a stop candidate of rank >= nb was passed over")
                    if defect != "stop candidate of rank >= nb added":
                        continue
                else:
                    log.events.add("a stop candidate of rank < nb became a hypothesis")
                hyps.add(seqs[src], float(sc), gen_len)
            else:
                new.append((sc, tok, src))
            if len(new) == nb:
                break
        assert len(new) == nb, "not enough non-stop candidates"
        if step == 0:
            log.events.add("step 0: every candidate from beam 0" if all(s == 0 for _, _, s in new) else "step 0: a dead beam survived")
        done = hyps.is_done(float(val[cand[0]]), gen_len)
        seqs = [seqs[s] + [t] for _, t, s in new]
        seens = [seens[s] | {t} for _, t, s in new]
        scores = torch.stack([sc for sc, _, _ in new])
        if done:
            break
    if not done:
        log.events.add("open beams finalised at max_length")
        for j in range(nb):
            hyps.add(seqs[j], float(scores[j]), len(seqs[j]))
    best = sorted(hyps.beams, key=lambda h: h[0]).pop()[1]
    return best


def run_beam(case: Case, dtype=torch.float32, defect=None, log=None, jitter=None) -> torch.Tensor:
    """beam cases -> the ids of the call (BeamSearchScorer.finalize: the best hypothesis of every utterance, the stop token behind it).
    jitter: a seed for `jittered` log-probabilities."""
    log = Log() if log is None else log
    stop = case.V - 1
    best = [_beam_unit(case, st, None if case.uniforms is None else case.uniforms[:, b], dtype, defect, log, jitter)
            for b, st in enumerate(unit_settings(case))]
    lens = [len(t) for t in best]
    if min(lens) != max(lens):
        log.events.add("the best hypotheses differ in length: padded output")
    n = min(max(lens) + 1, case.max_new)
    return torch.tensor([(t + [stop] * n)[:n] for t in best], dtype=torch.int64)


def restate(case: Case, dtype=torch.float32, defect=None, log=None, scores=None) -> torch.Tensor:
    if case.family == "beam":
        return run_beam(case, dtype, defect, log)
    return run_rows(case, dtype, defect, log, scores)


def expected_ids(case: Case) -> torch.Tensor:
    """what the engine must return: the oracle's ids under the tie rule; the restatement's for the two kinds of case the oracle cannot state"""
    return restate(case) if (case.cap or case.engine_thr) else oracle_ids(case)


# ----------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------
def _walk(n: int, B: int = 1) -> torch.Tensor:
    """u = (j + 0.5) / 16: sixteen evenly spaced points of the CDF, one per step; every row reads the same"""
    return ((torch.arange(n, dtype=torch.float64) + 0.5) / 16.0)[:, None].repeat(1, B)


def _case(name, family, V, values, st, why, B=1, max_new=4, rows=None, uniforms=None, row_max_new=None, radix=(None,), ties=False, cap=False,
          engine_thr=False, gate=True, walk=None, floor=FLOOR):
    return Case(f"{name}-V{V}", family, V, make_row(V, values, floor), B, max_new, st, rows, uniforms, row_max_new, tuple(radix), ties, cap,
                engine_thr, gate, None if walk is None else tuple(sorted(walk)), why)


def _both(V):
    """the sizes at which both top-k paths run (the radix select is the default of sample_kernel, the bisection of the beam kernels)"""
    return (0, 1) if V in (257, 8194) else (None,)


GREEDY = dict(do_sample=False)


def _greedy_cases():
    out = []
    for V in SIZES:
        out.append(_case("greedy-tie-0-and-last", "greedy", V, {0: 2.0, V - 1: 2.0}, GREEDY, "tie at the maximum between index 0 and V - 1 (the stop token): 0 wins",
                         ties=True, max_new=3))
        out.append(_case("greedy-tie-across-lanes", "greedy", V, {3: 2.0, 40: 2.0, 41: 1.75}, GREEDY, "tie between two lanes of wave 0", ties=True, max_new=3))
        out.append(_case("greedy-tie-across-waves", "greedy", V, {70: 2.0, 130: 2.0, 199: 2.0}, GREEDY, "tie between waves 1, 2 and 3", ties=True, max_new=3))
        out.append(_case("greedy-max-at-last", "greedy", V, {V - 1: 2.0, 5: 1.0}, GREEDY, "the maximum alone at V - 1", max_new=3))
        out.append(_case("greedy-max-before-stop", "greedy", V, {V - 3: 2.0, 5: 1.0}, GREEDY, "the maximum alone in the ragged tail", max_new=3))
        if V > 256:
            out.append(_case("greedy-tie-in-stride", "greedy", V, {6: 2.0, 262: 2.0} if V > 262 else {0: 2.0, 256: 2.0}, GREEDY,
                             "tie inside one thread's stride (i, i + 256)", ties=True, max_new=3))
            out.append(_case("greedy-max-at-255", "greedy", V, {255: 2.0, 5: 1.0}, GREEDY, "the maximum alone at 255", max_new=3))
            out.append(_case("greedy-max-at-256", "greedy", V, {256: 2.0, 5: 1.0}, GREEDY, "the maximum alone at 256", max_new=3))
    pen = dict(do_sample=False, repetition_penalty=2.0)
    for V in (200, 8194):
        out.append(_case("penalty-halves-positive", "greedy", V, {10: 4.0, 11: 3.0, 12: 1.25}, pen, "4 -> 2 -> 1, 3 -> 1.5: the order of the picks shows each halving",
                         max_new=6))
        out.append(_case("penalty-doubles-negative", "greedy", V, {10: -1.0, 11: -1.5, 12: -2.5}, pen, "-1 -> -2 -> -4, -1.5 -> -3: dividing would keep id 10 on top",
                         max_new=6))
        out.append(_case("penalty-leaves-zero", "greedy", V, {10: 0.0, 11: -0.0, 12: -0.25}, pen, "0.0 and -0.0 are unchanged, and tie: id 10 every step", ties=True,
                         max_new=4))
        out.append(_case("fake-prompt-penalised", "greedy", V, {1: 4.0, V - 2: 3.5, 20: 3.0}, pen,
                         "ids 1 and start_mel are penalised from step 0 on: id 1, the raw maximum, must not come first", max_new=5))
        out.append(_case("stop-wins-at-step-3", "greedy", V, {30: 8.0, 31: 7.0, 32: 6.0, V - 1: 5.0}, GREEDY,
                         "penalty 2 halves 8, 7, 6 in turn, then the stop token wins; forced stop tokens behind it; a penalty-1 row runs on; two rows capped",
                         B=4, max_new=6, rows=[dict(repetition_penalty=2.0), dict(repetition_penalty=1.0), dict(repetition_penalty=1.0),
                                               dict(repetition_penalty=2.0)], row_max_new=[6, 6, 2, 2]))
        out.append(_case("all-minus-inf-but-one", "greedy", V, {77: 0.0}, pen, "-inf everywhere but id 77", max_new=3, floor=NINF))
    return out


def _sample_cases():
    out = []
    for V in SIZES:
        tie8 = (7, 50, 51, 120, 190, 191, 192, V - 3)
        top = {9: 0.75, 100: 0.5, 150: 0.25}
        eq8 = {i: 0.0 for i in tie8}
        out.append(_case("topk-edge-8-way-tie", "sample", V, {**top, **eq8}, dict(do_sample=True, top_k=4), "an 8-way tie on the 4th value: all 11 are kept",
                         max_new=16, uniforms=_walk(16), radix=_both(V), ties=False, walk=tuple(top) + tie8))
        for tp, drop in ((0.75, 2), (0.5, 4), (0.875, 1)):
            if V in (200, 8194) or tp == 0.75:
                out.append(_case(f"top-p-{tp}-on-8-equal", "sample", V, eq8, dict(do_sample=True, top_k=8, top_p=tp),
                                 f"cum hits 1 - top_p exactly: <= removes {drop}, the lowest indices first", max_new=16, uniforms=_walk(16),
                                 radix=_both(V), ties=True, walk=tie8[drop:]))
    for V in (200, 8194):
        tie8 = (7, 50, 51, 120, 190, 191, 192, V - 3)
        keep = [dict(min_tokens_to_keep=1), dict(min_tokens_to_keep=2)]
        out.append(_case("min-keep-on-2-equal", "sample", V, {20: 1.0, 60: 1.0}, dict(do_sample=True, top_k=2, top_p=0.25), "cum 0.5 <= 0.75 removes id 20 unless two are kept",
                         B=2, rows=keep, max_new=4, uniforms=_walk(4, 2) * 4 % 1.0, ties=True))
        out.append(_case("min-keep-on-4-equal", "sample", V, {20: 1.0, 60: 1.0, 61: 1.0, 150: 1.0}, dict(do_sample=True, top_k=4, top_p=0.25),
                         "cum 0.25, 0.5, 0.75 <= 0.75 removes three, or two when two are kept", B=2, rows=keep, max_new=4, uniforms=_walk(4, 2) * 4 % 1.0, ties=True))
        eq5 = {i: 0.0 for i in tie8[:5]}
        out.append(_case("top-p-0.8-on-5-equal", "sample", V, eq5, dict(do_sample=True, top_k=5, top_p=0.8),
                         "cum[0] = 0.2f against the reference's 0.2f (<=: 4 kept) and the engine's 0.19999999f (5 kept)", max_new=16, uniforms=_walk(16),
                         ties=True, engine_thr=True, gate=False, walk=tie8[:5]))
        for T in (0.5, 2.0):
            out.append(_case(f"temperature-{T}", "sample", V, {10: 1.0, 11: 0.5, 12: 0.0, 13: -0.5, 14: -1.0}, dict(do_sample=True, top_k=4, temperature=T, repetition_penalty=2.0),
                             "penalty, then temperature, then top-k of 4 over five scores", max_new=8, uniforms=_walk(16)[1::2]))
        out.append(_case("uniform-edges-on-4-equal", "sample", V, {20: 1.0, 60: 1.0, 61: 1.0, 150: 1.0}, dict(do_sample=True, top_k=4),
                         "u = 0: the first kept id; 1 - 2^-53: the last; 0.25, 0.5, 0.75 sit on CDF steps, and cum > tgt is strict", max_new=5,
                         uniforms=torch.tensor([0.0, U_LAST, 0.25, 0.5, 0.75], dtype=torch.float64)[:, None], ties=False, walk=(20, 60, 61, 150)))
        typ = {10: 2.0, 11: 1.0, 12: 1.0, 13: 0.0, 14: 0.0, 15: -1.0, 16: -2.0}
        out.append(_case("typical-before-temperature", "sample", V, typ, dict(do_sample=True, top_k=8, typical_mass=0.5, temperature=2.0),
                         "the typical filter sees the untempered scores; pairs of equal scores tie in |-log p - H|", max_new=8, uniforms=_walk(16)[1::2], ties=False))
        out.append(_case("typical-greedy-ties", "greedy", V, typ, dict(do_sample=False, typical_mass=0.125, repetition_penalty=2.0),
                         "greedy over a typical-filtered row: the most probable token may be filtered out", max_new=6))
        out.append(_case("typical-mass-on-a-step", "sample", V, {i: 0.0 for i in tie8}, dict(do_sample=True, top_k=8, typical_mass=0.5),
                         "eight equal scores over -inf: the mass 0.5 ends exactly on the cumulative step 4/8, and every distance ties", max_new=8,
                         uniforms=_walk(16)[1::2], ties=False, floor=NINF, walk=tie8))
        sets = [dict(do_sample=False), dict(do_sample=True, top_k=4), dict(do_sample=True, top_k=8, top_p=0.5, temperature=2.0),
                dict(do_sample=True, top_k=8, typical_mass=0.5, repetition_penalty=2.0)]
        out.append(_case("four-setting-sets-one-row", "sample", V, {9: 0.75, 100: 0.5, 150: 0.25, **{i: 0.0 for i in tie8}}, GREEDY,
                         "the per-row table: four setting sets meet one row in one batch", B=4, rows=sets, max_new=8, uniforms=_walk(16, 4)[1::2], ties=True))
    for V in (257, 8449):
        tied = {i: 0.0 for i in range(20, 220)}
        out.append(_case("more-ties-than-slots", "sample", V, {5: 0.75, 230: 0.5, 240: 0.25, **tied}, dict(do_sample=True, top_k=4),
                         "200 scores tie on the 4th value under three higher ones: the three, then the 125 tied ones of lowest index", max_new=16,
                         uniforms=torch.cat([_walk(14), torch.tensor([[0.0], [U_LAST]], dtype=torch.float64)]), radix=_both(V), ties=True, cap=True))
    return out


def _beam_cases():
    out = []
    # two rows: the stop token second (rank < nb from step 0 on) and fourth (rank >= nb for 2 and 3 beams until penalties lift it)
    second = {10: 2.0, 11: 1.5, 12: 1.0, 13: 0.5, 14: 0.0, 15: -0.5, 16: -1.0, 17: -1.5}
    deep = {18 + i: -2.0 - 0.5 * i for i in range(8)}         # beam-sample draws 2 nb candidates: step 0 needs that many kept in beam 0 alone
    for V in (200, 8194):
        for nb in (2, 3, 4):
            # From the third step on two beams can hold the same tokens in another order: sums equal in exact arithmetic, not in floating point,
            # and not a structural tie.  Wider searches stop before such a pair can decide (the host file's margin gate and ulp jitter say where).
            short = 8 if nb == 2 else (3 if V == 200 else 2)
            for lp in (0.0, 1.0, 2.0):
                if V == 8194 and (nb, lp) not in ((2, 0.0), (3, 1.0), (4, 2.0)):
                    continue
                st = dict(num_beams=nb, length_penalty=lp, repetition_penalty=2.0)
                out.append(_case(f"beam{nb}-lp{lp}-stop-second", "beam", V, {**second, V - 1: 1.75}, st,
                                 "the stop token ranks second in every row: hypotheses from step 0 on, the heap fills, the done rule is asked", max_new=short, ties=True))
                out.append(_case(f"beam{nb}-lp{lp}-stop-fifth", "beam", V, {**second, V - 1: 0.25}, st,
                                 "the stop token ranks fifth: passed over at rank >= nb, a hypothesis once the penalty has lowered the others", max_new=8 if nb < 4 else 4,
                                 ties=True))
            if nb == 3:
                out.append(_case("beam3-two-stop-candidates-in-one-step", "beam", V, {10: 2.0, 11: 2.0, V - 1: 2.0},
                                 dict(num_beams=3, length_penalty=1.0, repetition_penalty=4.0),
                                 "ids 10, 11 and the stop token tie on top: step 1 holds the stop token from two beams, at a rank below nb and at one "
                                 "at or above it; the second must not become a hypothesis", max_new=2, ties=True))
            st1 = dict(num_beams=nb, length_penalty=1.0, repetition_penalty=1.0)
            out.append(_case(f"beam{nb}-ties-across-beams", "beam", V, second, st1,
                             "penalty 1: after two steps a + b and b + a are equal bits in two beams, and the floor ties 190 times in every row; no stop: open beams finalised",
                             max_new=4, ties=True))
            u = torch.rand(6, 2, 2 * nb, dtype=torch.float64, generator=torch.Generator().manual_seed(40 + nb))
            u[0, 0, :], u[1, 0, :] = 0.0, U_LAST
            groups = [dict(do_sample=True, length_penalty=0.0), dict(do_sample=True, length_penalty=2.0)]
            out.append(_case(f"beam{nb}-sample-group-table", "beam", V, {**second, **deep, V - 1: 1.75},
                             dict(num_beams=nb, top_k=12, top_p=0.875, temperature=2.0, repetition_penalty=2.0),
                             "beam-sample, draws without replacement with u = 0 and u next to 1, two groups with their own length penalty", B=2, rows=groups,
                             max_new=2, uniforms=u, ties=True))
            out.append(_case(f"beam{nb}-search-group-table", "beam", V, {**second, V - 1: 1.75}, dict(num_beams=nb, repetition_penalty=2.0),
                             "two groups of one batch under length penalty 0 and 2: best hypotheses of different lengths", B=2,
                             rows=[dict(length_penalty=0.0), dict(length_penalty=2.0)], max_new=short, ties=True))
    for V in (257, 8449):
        out.append(_case("beam3-more-ties-than-slots", "beam", V, {i: 1.0 for i in range(20, 120)}, dict(num_beams=3, length_penalty=1.0, repetition_penalty=1.0),
                         "100 scores tie on the maximum of every row, more than the 64 survivor slots: the lowest indices win, as without a cap", max_new=3,
                         radix=_both(V), ties=True))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _greedy_cases() + _sample_cases() + _beam_cases()
    assert len({c.name for c in out}) == len(out)
    for c in out:
        assert c.max_new <= 16 and c.B <= 4, c.name
    return tuple(out)


def by_name(name: str) -> Case:
    return next(c for c in cases() if c.name == name)
