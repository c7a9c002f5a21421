"""GPU tests of the flow-matching decoder on RAGGED packed batches against an oracle that shares nothing with the engine: `oracle/s2mel_oracle.py`
run in f64, one utterance per call (batch 1, the utterance's own length: how the reference itself is called).

Every other ragged-batch test of the fp32x3 / fp32 modes compares two engine variants with `torch.equal`; the variants share the packed-row tables,
the tile store, the tap-mode source rows, the RoPE epilogue and the row-mapped residual, so an error in any of those passes them all.  Here:

(a) the whole 3-step Euler solve, per utterance, in the fp32 mode and in the fp32x3 mode as shipped (tail layout, `s2mel_prune_last`, the row-mapped
    `EPI_RESIDUAL_SRC` epilogue, `x3_attn_skip`, the 8-wave GEMM, plane operands), with 8 products and with the two last-layer options off; the
    bf16 mode on the same batches, with a bound on the frames next to the sequence boundaries beside the RMS one;
(b) ONE estimator call stage by stage: the image of every labelled stage (`itts_s2mel_set_trace` / `itts_s2mel_set_capture`) against the oracle's
    tap of the same stage and layer, which reaches every fused GEMM epilogue (QKV + RoPE, SwiGLU, tap-mode conv + gate, res/skip, residual) on its own.

Batches (tests/test_oracle_s2mel.py::RAGGED): the smallest that put several sequences into one 128-row m-tile and one 256-query block, make sequences
start and end mid-tile and hit both edges of the 64-key tile.  Engine: production widths (hidden 512, 8 heads, SwiGLU 1536, WaveNet 512, k = 5),
3 DiT layers (one U-ViT skip), 3 WaveNet layers of dilation 1, 2, 4 (14-frame halo).

Tolerances.  tests/test_oracle_s2mel.py::test_f32_oracle_vs_f64_oracle_on_the_ragged_batch measures what f32 arithmetic itself costs on these shapes:
the CPU f32 oracle is within max 1.4e-5 / rms 2.9e-6 of the f64 oracle (worst utterance of the measurement the bounds were set from).  The solve's
bounds are the project's F32_TOL = 1e-4 on max|d| (7x that 1.4e-5) and 2e-5 on rms(d) (the same 7x over 2.9e-6).  Per stage: max|d| <= 1e-4 x
rms(reference stage), and rms(d) <= 4 x the CPU f32 oracle's rms error at that same stage and layer (+ 1e-7 x rms(reference) where the f32 oracle is
exact, e.g. a masked row) -- the comparand is the CPU oracle, never the engine; the 4 allows for the MFMA tile order against the CPU BLAS order (the
project's GEMM unit tests hold the x3 kernels to 1.25-2x the native f32 error).  Measured figures: profiles/r09a/."""
import ctypes as C

import pytest
import torch

from oracle import s2mel_oracle as S
from tests.test_gpu_s2mel import BF16_EULER_RMS, F32_TOL, args_of
from tests.test_oracle_s2mel import RAGGED, RAGGED_STEPS, RAGGED_T, ragged_estimator_inputs, ragged_inputs, ragged_model, ragged_solve, ragged_taps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SOLVE_RMS_TOL = 2e-5
STAGE_MAX_REL = 1e-4               # max|d| of a stage, in units of the reference stage's rms
STAGE_RMS_FACTOR = 4.0             # rms(d) of a stage, in units of the CPU f32 oracle's rms error at the same stage
STAGE_RMS_FLOOR = 1e-7             # ... + this x rms(reference stage)
EDGE = 16                          # bf16: the first and the last EDGE generated frames of every sequence
# bf16 max|d| over those frames.  First GPU run of the engine (profiles/r09a/ragged_f64_before.log): 0.016-0.041 per utterance, the worst over both
# batches, both guidance rates and every utterance 0.0413 (`tail`, guidance 0.7, the row without a prompt); the bound is 2x that = 0.0826.  (With the
# f64-built RoPE table, profiles/r09a/ragged_f64.log: worst 0.0407, the same row.)  A reflect source taken from a neighbouring sequence or a mask row
# off by one changes these frames by O(1) (the mel has rms 1.5-1.8), which the 0.03 RMS bound over a few hundred frames dilutes.
BF16_EDGE_MEASURED = 0.0413
BF16_EDGE_MAX = 2 * BF16_EDGE_MEASURED

# mode -> (engine precision, options for the call)
MODES = {"fp32": ("fp32", {}),
         "fp32x3": ("fp32x3", {}),
         "fp32x3-8": ("fp32x3", dict(x3_products=8)),
         "fp32x3-full-last-layer": ("fp32x3", dict(s2mel_prune_last=0, x3_attn_skip=0))}


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def engines():
    """one engine per precision, built on first use"""
    from indextts_amd import s2mel
    cfg, sd = ragged_model()
    made = {}

    def get(precision):
        if precision not in made:
            made[precision] = s2mel.CFM(args_of(cfg), precision=precision, device=DEV)
            made[precision].load_state_dict(sd)
        return made[precision]
    return get


def _solve(m, name, rate, opts):
    from indextts_amd import _lib
    T, Tp, xl = RAGGED[name]
    x, mu, prompt, style = ragged_inputs(name)
    with _lib.option_scope(**opts):
        return m.solve_euler(x.clone(), torch.tensor(xl), prompt, mu, style, None, torch.linspace(0, 1, RAGGED_STEPS + 1), rate,
                             prompt_lens=Tp, frame_lens=T).cpu()


def _where(d, T, Tp, xl):
    """the worst element of d (C, T) and where its frame lies in the sequence: what tells a boundary bug from a precision one"""
    idx = int(d.abs().argmax())
    c, f = divmod(idx, d.shape[1])
    return (f"worst |d| {float(d.abs().max()):.3e} at frame {f} channel {c}: {f} frames after the sequence's start, {f - Tp} after the prompt's end "
            f"({Tp}), {T - 1 - f} before the last frame ({T - 1}), {xl - 1 - f} before the last valid frame ({xl - 1})")


def _check_layout(y, name):
    """what solve_euler promises around the generated frames: prompt frames are held at 0 (flow_matching.py:112) and `_unpack_rows` leaves the
    frames past a row's frame_lens of the padded (B, C, Tmax) output at 0"""
    T, Tp, _ = RAGGED[name]
    assert y.shape == (len(T), 80, max(T))
    for u in range(len(T)):
        assert float(y[u, :, : Tp[u]].abs().sum()) == 0.0, (name, u, "prompt frames are not 0")
        assert float(y[u, :, T[u]:].abs().sum()) == 0.0, (name, u, "frames past T[u] are not 0")


# ----------------------------------------------------------------------------------------------------------------
# (a) the whole solve
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [0.7, 0.0])
@pytest.mark.parametrize("name", ["tail", "no_tail"])
@pytest.mark.parametrize("mode", list(MODES))
def test_solve_vs_f64_oracle_per_utterance(engines, mode, name, rate):
    """3 Euler steps, guidance on (two branches) and off.  Per utterance on frames [:T[u]] (row 0 of `tail` includes its 9 masked frames: the
    reference computes them, and so does the engine with frame_lens = T): max|d| <= F32_TOL, rms(d) <= 2e-5 (module docstring); prompt frames
    and the padding past T[u] exactly 0."""
    prec, opts = MODES[mode]
    T, Tp, xl = RAGGED[name]
    y = _solve(engines(prec), name, rate, opts)
    ref, f32 = ragged_solve(name, rate, torch.float64), ragged_solve(name, rate, torch.float32)
    _check_layout(y, name)
    bad = []
    for u in range(len(T)):
        d = y[u, :, : T[u]].double() - ref[u][0]
        o = f32[u][0].double() - ref[u][0]
        mx, r = float(d.abs().max()), _rms(d)
        print(f"solve  {name:7s} cfg {rate:.1f} {mode:22s} utt {u} (T {T[u]:3d} prompt {Tp[u]:3d}): max|d| {mx:.3e} rms {r:.3e} | CPU f32 oracle "
              f"max|d| {float(o.abs().max()):.3e} rms {_rms(o):.3e} | output rms {_rms(ref[u]):.3f}")
        assert bool(torch.isfinite(y[u]).all()) and _rms(y[u, :, Tp[u]: T[u]]) > 0.1
        if mx > F32_TOL or r > SOLVE_RMS_TOL:
            bad.append(f"{mode} {name} cfg {rate} utterance {u} (T {T[u]}): rms {r:.3e}; " + _where(d, T[u], Tp[u], xl[u]))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("rate", [0.7, 0.0])
@pytest.mark.parametrize("name", ["tail", "no_tail"])
def test_bf16_solve_rms_and_boundary_frames(engines, name, rate):
    """The bf16 mode on the same batches: rms(d) <= BF16_EULER_RMS per utterance, and max|d| <= BF16_EDGE_MAX over the first and the last 16
    generated frames of every sequence (the frames a wrong reflect source, tap row or mask row reaches first; bound: see BF16_EDGE_MAX)."""
    T, Tp, xl = RAGGED[name]
    y = _solve(engines("bf16"), name, rate, {})
    ref = ragged_solve(name, rate, torch.float64)
    _check_layout(y, name)
    bad = []
    for u in range(len(T)):
        d = y[u, :, : T[u]].double() - ref[u][0]
        r = _rms(d)
        edge = d.clone()
        edge[:, Tp[u] + EDGE: T[u] - EDGE] = 0                        # (a 2-frame sequence is all edge)
        edge[:, : Tp[u]] = 0
        e = float(edge.abs().max())
        print(f"solve  {name:7s} cfg {rate:.1f} {'bf16':22s} utt {u} (T {T[u]:3d} prompt {Tp[u]:3d}): rms {r:.4f} (bound {BF16_EULER_RMS}) "
              f"max|d| over the {EDGE} first / last generated frames {e:.4f} (bound {BF16_EDGE_MAX:.4f}), over all frames {float(d.abs().max()):.4f}")
        if not (r <= BF16_EULER_RMS and e <= BF16_EDGE_MAX):
            bad.append(f"bf16 {name} cfg {rate} utterance {u} (T {T[u]}): rms {r:.4f}; boundary frames: " + _where(edge, T[u], Tp[u], xl[u]))
    assert not bad, "\n".join(bad)


# ----------------------------------------------------------------------------------------------------------------
# (b) one estimator call, stage by stage
# ----------------------------------------------------------------------------------------------------------------
# trace label -> (group, oracle tap key; {i} = the label's n-th occurrence mapped to a layer).  All of these are f32 rows [n_tok][C] in the fp32 and
# fp32x3 modes (fp32x3 keeps Q as f32 rows: flash_attn_x3_kernel splits the queries in registers; only K / V^T and the adaptive-norm outputs are planes).
STAGES = {
    "x_in GEMM -> X": ("head", "x_in"),
    "wqkv -> Q": ("dit", "dit.{i}.q"),
    "attention -> AO": ("dit", "dit.{i}.ao"),
    "wo GEMM -> X": ("dit", "dit.{i}.x_attn"),
    "w13 + SwiGLU -> FC": ("dit", "dit.{i}.swiglu"),
    "w2 GEMM -> X": ("dit", "dit.{i}.x_ffn"),
    "skip_in GEMMs -> X": ("dit", "dit.{i}.skip_in"),
    "final ada_rmsnorm -> HB": ("head", "final_norm"),
    "skip_linear -> X2": ("head", "skip_linear"),
    "conv1 -> WX": ("head", "conv1"),
    "wavenet in_layer + gate -> FC": ("wn", "wn.{i}.gate"),
    "wavenet res_skip -> WX": ("wn", "wn.{i}.x"),
    "wavenet res_skip -> OUT": ("wn", "wn.{i}.skip"),
    "final_layer -> FC": ("head", "final_layer"),
    "conv2 -> output": ("head", "conv2"),
}
# traced stages that are NOT compared, by name (a label in neither table fails the test: a new or renamed stage needs a decision)
NOT_COMPARED = {
    "cast_pad(x) -> XA": "the input x, zero-padded to the GEMM's K: no arithmetic",
    "ada_rmsnorm(attn) -> HB": "no oracle tap (its consumer `wqkv -> Q` is compared)",
    "ada_rmsnorm(ffn) -> HB": "no oracle tap (its consumer `w13 + SwiGLU -> FC` is compared)",
    "ada_rmsnorm(attn) -> HB planes": "fp32x3: three bf16 planes in fragment order (its consumer `wqkv -> Q` is compared)",
    "ada_rmsnorm(ffn) -> HB planes": "fp32x3: three bf16 planes in fragment order (its consumer `w13 + SwiGLU -> FC` is compared)",
    "wqkv -> K": "head-major key cache, bf16 planes in fp32x3 (K after RoPE reaches `attention -> AO`)",
    "wqkv -> V^T": "transposed head-major value cache, bf16 planes in fp32x3 (reaches `attention -> AO`)",
}


def _layer_of(label, occurrence, cfg):
    if label == "skip_in GEMMs -> X":                                  # only the layers past the middle receive a skip
        return cfg.depth // 2 + 1 + occurrence
    return occurrence


class _StageCapture:
    """ctypes plumbing of the engine's stage trace: `images(prefix, call)` runs `call()` once with a copy of every stage output whose label starts
    with `prefix` and returns [(label, occurrence of the label in the call, f32 CPU tensor of the image)]."""

    def __init__(self, m, nbytes=160 << 20, cap=512):
        from indextts_amd import _lib
        self._lib, self.L, self.m, self.cap = _lib, _lib.lib(), m, cap
        self.words = torch.zeros(cap, dtype=torch.int64, device=DEV)
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.check(self.L.itts_s2mel_set_trace(m._h, _lib.ptr(self.words), cap), "itts_s2mel_set_trace")

    def labels(self):
        n = self.L.itts_s2mel_trace_count(self.m._h)
        assert 0 < n == self.L.itts_s2mel_trace_wanted(self.m._h) <= self.cap, "the stage trace stopped at its capacity"
        return [(self.L.itts_s2mel_trace_label(self.m._h, i) or b"?").decode() for i in range(n)]

    def images(self, prefix, call):
        _lib, L, h = self._lib, self.L, self.m._h
        _lib.check(L.itts_s2mel_set_capture(h, _lib.ptr(self.buf), self.buf.numel(), prefix.encode()), "itts_s2mel_set_capture")
        call()
        torch.cuda.synchronize()
        out, seen = [], {}
        for i, label in enumerate(self.labels()):
            k = seen.get(label, 0)
            seen[label] = k + 1
            if not label.startswith(prefix):
                continue
            nb = C.c_size_t(0)
            off = L.itts_s2mel_capture_offset(h, i, C.byref(nb))
            assert off >= 0 and nb.value % 4 == 0, f"stage {i} '{label}' was not captured (capture buffer too small?)"
            out.append((label, k, self.buf[off: off + nb.value].clone().view(torch.float32).cpu()))
        return out

    def close(self):
        self._lib.check(self.L.itts_s2mel_set_capture(self.m._h, None, 0, None), "itts_s2mel_set_capture")
        self._lib.check(self.L.itts_s2mel_set_trace(self.m._h, None, 0), "itts_s2mel_set_trace")


def _stage_ids(v):
    return v.replace(" -> ", "->").replace(" ", "_")


def _estimator_call(m):
    T, _, xl = RAGGED["tail"]
    B = len(T)
    _, mu, _, style = ragged_inputs("tail")
    x, px = ragged_estimator_inputs("tail")
    return lambda: m.estimator(torch.cat([x, x]), torch.cat([px, torch.zeros_like(px)]), torch.tensor(xl), torch.full((2 * B,), RAGGED_T),
                               torch.cat([style, torch.zeros_like(style)]), torch.cat([mu, torch.zeros_like(mu)]), frame_lens=T + T)


@pytest.mark.parametrize("mode", ["fp32", "fp32x3"])
def test_every_traced_stage_is_compared_or_named(engines, mode):
    """The stage trace of the estimator call below holds every label of STAGES (a renamed label cannot empty the stage tests) and nothing that is in
    neither STAGES nor NOT_COMPARED (a new stage needs a decision); the stages left out are printed by name with the reason."""
    from indextts_amd import _lib
    prec, opts = MODES[mode]
    m = engines(prec)
    cap = _StageCapture(m, nbytes=256)
    try:
        with _lib.option_scope(**opts):
            _estimator_call(m)()
            torch.cuda.synchronize()
            traced = cap.labels()
    finally:
        cap.close()
    for label in sorted(set(traced) & set(NOT_COMPARED)):
        print(f"stage  {mode:7s} '{label}': not compared -- {NOT_COMPARED[label]}")
    assert not set(traced) - set(STAGES) - set(NOT_COMPARED), sorted(set(traced) - set(STAGES) - set(NOT_COMPARED))
    assert not set(STAGES) - set(traced), sorted(set(STAGES) - set(traced))


@pytest.mark.parametrize("label", list(STAGES), ids=_stage_ids)
@pytest.mark.parametrize("mode", ["fp32", "fp32x3"])
def test_estimator_stage_vs_f64_oracle(engines, mode, label):
    """One CFG-stacked estimator call on the `tail` batch (t = 0.3, frame_lens = T: the full layout, every row present, 2 x 1358 packed rows) with the
    images of every stage carrying `label` captured (one per layer).  Packed rows are mapped to (branch, sequence, frame) by the engine's own `_tables`
    and `_unpack_rows`; the reference is the f64 oracle's tap of the same stage and layer, called per utterance, the null branch by a second call on
    zeroed conditioning.  Gates per stage and layer over every row of the batch (module docstring): max|d| <= 1e-4 x rms(reference), rms(d) <= 4 x
    the CPU f32 oracle's + 1e-7 x rms(reference).  The image must be f32 rows of the tap's width, and there must be one per expected layer.

    Rows at masked frames (row 0, t >= x_lens = 696) are compared at EVERY stage: the reference defines them all -- masked frames are never keys,
    but they are queries and run through every row-wise stage; `wn.{i}.x` is masked to 0 there on both sides, the running skip sum is traced
    before its mask on both sides, and the final layer sees 0 + res_projection there on both sides.

    Measured (profiles/r09a/ragged_f64.log).  rms(d) is 1.00-1.20 x the CPU f32 oracle's at every stage but `wqkv -> Q`, 0.4-0.8 x (the oracle's f32 RoPE table is the coarser one), and
    `x_in GEMM -> X`, 1.8 x (3.9e-7
    against 2.1e-7: the engine sums the step-invariant columns in a GEMM of their own and adds the x columns to the rounded result); nothing comes
    near the 4.  max|d| is 0.5-7.0e-5 x rms(reference) (`wqkv -> Q`: 0.5-1.3e-5).

    What this test found (profiles/r09a/ragged_f64_before.log): with the RoPE table built in f32 on the device, as the reference's formula reads,
    `wqkv -> Q` missed the max gate in both modes -- 1.63 / 1.77 / 1.69 e-4 x rms(reference) at layers 0 / 1 / 2 in fp32, 1.63 / 1.74 / 1.71 e-4 in
    fp32x3, the CPU f32 oracle itself at 0.90 / 1.02 / 0.78 e-4.  Not a boundary error: the worst elements were frames 686 and 697 of the 705-frame
    row, channels 2, 259 and 322, i.e. always rotation pair 1 of a head (frequency 10000^(-1/32), the fastest that is not exactly 1) at the largest
    positions of the batch, in both branches: at position 700 the f32 product position x frequency is off by up to 700 x 2^-24 = 4e-5 rad and the
    device's f32 `pow` adds as much through the frequency, times |q| of 3-4.  `CFM._rope` now forms the angles in f64 and rounds the table once."""
    from indextts_amd import _lib, s2mel
    prec, opts = MODES[mode]
    m = engines(prec)
    cfg, _ = ragged_model()
    T, Tp, xl = RAGGED["tail"]
    B, Tm = len(T), max(T)
    group, key = STAGES[label]
    ref, f32 = ragged_taps("tail", torch.float64), ragged_taps("tail", torch.float32)
    tabs, n_tok, _ = m._tables(T + T, torch.tensor(xl + xl), 1)
    sq, fr = tabs["tok_seq"].long().cpu(), tabs["tok_t"].long().cpu()
    assert n_tok == 2 * sum(T)
    cap = _StageCapture(m)
    try:
        with _lib.option_scope(**opts):
            images = cap.images(label, _estimator_call(m))
    finally:
        cap.close()
    layers, bad = [], []
    for lab, k, img in images:
        assert lab == label, (lab, label)
        i = _layer_of(lab, k, cfg)
        tap = key.format(i=i)
        width = ref[0][0][tap].shape[-1]
        assert img.numel() == n_tok * width, f"'{lab}' [{k}]: {img.numel() * 4} bytes are not {n_tok} f32 rows of {width}"
        got = s2mel.CFM._unpack_rows(img.view(n_tok, width), sq, fr, 2 * B, Tm).transpose(1, 2)          # (2B, Tmax, C)
        se_d = se_o = se_r = 0.0
        n = 0
        worst = (-1.0, None)
        for br in (0, 1):
            for u in range(B):
                r64 = ref[br][u][tap][0]
                d = got[br * B + u, : T[u]].double() - r64
                o = f32[br][u][tap][0].double() - r64
                se_d += float(d.pow(2).sum())
                se_o += float(o.pow(2).sum())
                se_r += float(r64.pow(2).sum())
                n += d.numel()
                if not float(d.abs().max()) <= worst[0]:                # (a NaN lands here too)
                    worst = (float(d.abs().max()), (br, u, d))
        rms_d, rms_o, rms_r = (se_d / n) ** 0.5, (se_o / n) ** 0.5, (se_r / n) ** 0.5
        layers.append(i)
        print(f"stage  {mode:7s} {lab:30s} layer {i}: reference rms {rms_r:.3e} | max|d| {worst[0]:.3e} = {worst[0] / rms_r:.2e} x rms(ref) "
              f"| rms(d) {rms_d:.3e}, CPU f32 oracle {rms_o:.3e}, ratio {rms_d / max(rms_o, 1e-300):.2f}")
        if not (worst[0] <= STAGE_MAX_REL * rms_r and rms_d <= STAGE_RMS_FACTOR * rms_o + STAGE_RMS_FLOOR * rms_r):
            br, u, d = worst[1]
            bad.append(f"{mode} '{lab}' layer {i}: max|d| {worst[0]:.3e} (bound {STAGE_MAX_REL * rms_r:.3e}), rms(d) {rms_d:.3e} (bound "
                       f"{STAGE_RMS_FACTOR * rms_o + STAGE_RMS_FLOOR * rms_r:.3e}); utterance {u} branch {('cond', 'null')[br]}: "
                       + _where(d.t(), T[u], Tp[u], xl[u]))
    want = {"head": [0], "wn": list(range(cfg.wavenet_layers)), "dit": list(range(cfg.depth))}[group]
    if label == "skip_in GEMMs -> X":
        want = list(range(cfg.depth // 2 + 1, cfg.depth))
    assert layers == want, (label, layers, want)
    assert not bad, "\n".join(bad)
