"""Oracle for the first "next" row (SURVEY.md section 8f-1, s2mel CFM / DiT) vs the fixture minted from the reference's own
CFM / DiT classes (tools/make_golden_s2mel.py): these tests pin the oracle only (the engine's parity tests are tests/test_gpu_s2mel*.py).
The second half holds the ragged batches, their inputs and the oracle's f32 / f64 results that tests/test_gpu_s2mel_ragged_f64.py shares, and
measures the f32 oracle against the f64 one: the yardstick of that file's tolerances."""
import functools
import os

import numpy as np
import torch

from oracle import s2mel_oracle as S


def load(golden_dir):
    z = np.load(os.path.join(golden_dir, "s2mel_cfm.npz"))
    c = [int(v) for v in z["cfg"]]
    cfg = S.S2MelConfig(hidden_dim=c[0], num_heads=c[1], depth=c[2], in_channels=c[3], content_dim=c[4], style_dim=c[5],
                        wavenet_hidden=c[6], wavenet_layers=c[7], wavenet_kernel=c[8], wavenet_dilation_rate=c[9])
    return z, cfg, S.synth_weights(cfg, int(z["seed"]))


def test_estimator_matches_reference(golden_dir):
    z, cfg, sd = load(golden_dir)
    x = torch.from_numpy(z["z"])
    T, Tp = x.shape[-1], z["prompt"].shape[-1]
    px = torch.zeros_like(x)
    px[..., :Tp] = torch.from_numpy(z["prompt"])
    style, mu = torch.from_numpy(z["style"]), torch.from_numpy(z["mu"])
    with torch.no_grad():
        d = S.dit_forward(sd, cfg, torch.cat([x, x]), torch.cat([px, torch.zeros_like(px)]), torch.from_numpy(z["x_lens"]),
                          torch.from_numpy(z["t"]), torch.cat([style, torch.zeros_like(style)]), torch.cat([mu, torch.zeros_like(mu)]))
    assert d.shape == (2, cfg.in_channels, T)
    np.testing.assert_allclose(d.numpy(), z["estimator_out"], rtol=0, atol=2e-5)


def test_euler_solver_matches_reference(golden_dir):
    z, cfg, sd = load(golden_dir)
    with torch.no_grad():
        y = S.cfm_solve_euler(sd, cfg, torch.from_numpy(z["z"]), torch.from_numpy(z["x_lens"]), torch.from_numpy(z["prompt"]),
                              torch.from_numpy(z["mu"]), torch.from_numpy(z["style"]), int(z["n_steps"]), float(z["cfg_rate"]))
    np.testing.assert_allclose(y.numpy(), z["euler_out"], rtol=0, atol=2e-5)
    Tp = z["prompt"].shape[-1]
    assert float(y[..., :Tp].abs().max()) == 0.0                      # prompt frames are held at zero (flow_matching.py:112)


def test_padded_keys_do_not_reach_valid_frames(golden_dir):
    """sequence_mask semantics: frames beyond x_lens are never attended to; the transformer and WaveNet masks together make
    the valid frames independent of what the padded input frames hold except through the (unmasked) reflect-padded convs'
    3 * 4-frame reach at the boundary."""
    z, cfg, sd = load(golden_dir)
    x = torch.from_numpy(z["z"]).clone()
    T = x.shape[-1]
    n = int(z["x_lens"][0])
    px = torch.zeros_like(x)
    style, mu = torch.from_numpy(z["style"]), torch.from_numpy(z["mu"])
    t = torch.tensor([0.5])
    with torch.no_grad():
        a = S.dit_forward(sd, cfg, x, px, torch.tensor([n]), t, style, mu)
        x2 = x.clone()
        x2[..., n:] += 3.0
        b = S.dit_forward(sd, cfg, x2, px, torch.tensor([n]), t, style, mu)
    reach = sum((cfg.wavenet_kernel - 1) // 2 * cfg.wavenet_dilation_rate ** i for i in range(cfg.wavenet_layers)) + 1
    assert float((a - b)[..., : n - reach].abs().max()) < 1e-4


def load_prod(golden_dir):
    """Third fixture (tools/make_golden_s2mel.py::main_prod): the PRODUCTION widths (DiT 13 x 512 x 8 heads, WaveNet 8 x 512) and solve depth (25
    CFG Euler steps) run through the reference's classes; `mu` is regenerated from the seed (its sum is the fixture's drift check)."""
    z = np.load(os.path.join(golden_dir, "s2mel_cfm_prod.npz"))
    cfg = S.S2MelConfig()
    seed, T = int(z["seed"]), int(z["T"])
    mu = torch.randn(1, T, cfg.content_dim, generator=torch.Generator().manual_seed(seed + 2))
    assert abs(float(mu.double().sum()) - float(z["mu_sum"])) < 1e-6, "torch's CPU generator no longer reproduces the fixture's mu"
    return z, cfg, S.synth_weights(cfg, seed), mu


def test_production_widths_estimator_and_25_step_solve_match_reference(golden_dir):
    z, cfg, sd, mu = load_prod(golden_dir)
    x, prompt, style, x_lens = (torch.from_numpy(z[k]) for k in ("z", "prompt", "style", "x_lens"))
    Tp = prompt.shape[-1]
    px = torch.zeros_like(x)
    px[..., :Tp] = prompt
    with torch.no_grad():
        d = S.dit_forward(sd, cfg, torch.cat([x, x]), torch.cat([px, torch.zeros_like(px)]), x_lens, torch.full((2,), float(z["t"])),
                          torch.cat([style, torch.zeros_like(style)]), torch.cat([mu, torch.zeros_like(mu)]))
        y = S.cfm_solve_euler(sd, cfg, x, x_lens, prompt, mu, style, int(z["n_steps"]), float(z["cfg_rate"]))
    np.testing.assert_allclose(d.numpy(), z["estimator_out"], rtol=0, atol=3e-5)
    np.testing.assert_allclose(y.numpy(), z["euler_out"], rtol=0, atol=3e-5)
    assert float(y[..., :Tp].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------
# f64 mode and stage taps; the ragged batches shared with tests/test_gpu_s2mel_ragged_f64.py
# ----------------------------------------------------------------------------------------------------------------
# name -> (frame lengths T, prompt lengths Tp, valid lengths x_lens).  Packed, the four `tail` sequences start at rows 0, 705, 972 and 1069: three
# of them share the m-tile of rows 1024..1151 and the 256-query block from 768 on, every one starts and ends mid-tile, and T % 64 = 1, 11, 33, 33
# (x_lens 696 % 64 = 56) puts the last keys at both edges of the 64-key tile; row 0 carries 9 masked frames as the production fixture does.
# `no_tail`: the second row's tail would be one WaveNet conv's padding, so the engine's solve runs without a tail layout.
RAGGED = {"tail": ([705, 267, 97, 289], [200, 0, 9, 60], [696, 267, 97, 289]),
          "no_tail": ([391, 24], [140, 22], [391, 24])}
RAGGED_STEPS = 3
RAGGED_T = 0.3                                  # the timestep of the single estimator call


@functools.lru_cache(maxsize=None)
def ragged_model(dtype=torch.float32):
    """production widths (hidden 512, 8 heads, SwiGLU 1536, WaveNet 512, k = 5), 3 DiT layers (one U-ViT skip), 3 WaveNet layers, 14-frame halo"""
    cfg = S.S2MelConfig(depth=3, wavenet_layers=3, wavenet_dilation_rate=2)
    return cfg, {k: v.to(dtype) for k, v in S.synth_weights(cfg, 5).items()}


@functools.lru_cache(maxsize=None)
def ragged_inputs(name):
    """(x, mu, prompt, style) of the padded batch, f32, seeded; frames past T[u] hold noise too (nothing may read them)"""
    cfg, _ = ragged_model()
    T, Tp, _ = RAGGED[name]
    g = torch.Generator().manual_seed(6)
    B, Tm = len(T), max(T)
    x = torch.randn(B, 80, Tm, generator=g)
    mu = torch.randn(B, Tm, cfg.content_dim, generator=g)
    prompt = torch.randn(B, 80, max(max(Tp), 1), generator=g) * 0.5 - 1.0
    style = torch.randn(B, cfg.style_dim, generator=g)
    return x, mu, prompt, style


@functools.lru_cache(maxsize=None)
def ragged_solve(name, rate, dtype=torch.float64):
    """The oracle's 3-step solve of every utterance ALONE (batch 1, T[u] frames, its own x_lens: how the reference is called), computed in `dtype`
    from the f32 inputs: a list of (1, 80, T[u]) tensors.  Cached: shared by every test of the process, never modified."""
    cfg, sd = ragged_model(dtype)
    T, Tp, xl = RAGGED[name]
    x, mu, prompt, style = (t.to(dtype) for t in ragged_inputs(name))
    out = []
    with torch.no_grad():
        for u in range(len(T)):
            out.append(S.cfm_solve_euler(sd, cfg, x[u:u + 1, :, : T[u]], torch.tensor([xl[u]]), prompt[u:u + 1, :, : Tp[u]], mu[u:u + 1, : T[u]],
                                         style[u:u + 1], RAGGED_STEPS, rate))
    return out


def ragged_estimator_inputs(name):
    """x with the prompt frames zeroed and prompt_x holding the prompt there (what the solver feeds the estimator), (B, 80, Tmax) each"""
    T, Tp, _ = RAGGED[name]
    x, _, prompt, _ = ragged_inputs(name)
    x, px = x.clone(), torch.zeros_like(x)
    for u in range(len(T)):
        px[u, :, : Tp[u]] = prompt[u, :, : Tp[u]]
        x[u, :, : Tp[u]] = 0
    return x, px


@functools.lru_cache(maxsize=None)
def ragged_taps(name, dtype=torch.float64):
    """Stage taps of ONE estimator call at t = RAGGED_T per utterance and CFG branch: taps[branch][u] = {key: (1, T[u], C)}, branch 0 the
    conditional call, branch 1 a second call on zeroed prompt_x / style / mu (the null branch of the CFG-stacked batch)."""
    cfg, sd = ragged_model(dtype)
    T, _, xl = RAGGED[name]
    _, mu, _, style = ragged_inputs(name)
    x, px = ragged_estimator_inputs(name)
    out = ([], [])
    with torch.no_grad():
        for u in range(len(T)):
            a = [t.to(dtype) for t in (x[u:u + 1, :, : T[u]], px[u:u + 1, :, : T[u]], style[u:u + 1], mu[u:u + 1, : T[u]])]
            for br in (0, 1):
                taps = {}
                xx, pp, ss, mm = a if br == 0 else (a[0], torch.zeros_like(a[1]), torch.zeros_like(a[2]), torch.zeros_like(a[3]))
                S.dit_forward(sd, cfg, xx, pp, torch.tensor([xl[u]]), torch.full((1,), RAGGED_T, dtype=dtype), ss, mm, taps=taps)
                out[br].append(taps)
    return out


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


def test_f32_default_is_bit_identical_with_taps_and_f64_follows_the_inputs(golden_dir):
    """`taps` only records: the f32 result with a taps dict is the result without, bit for bit (estimator and, through it, the solve); every
    documented key is there as (B, T, C); inputs cast to f64 give an f64 result close to the f32 one; taps with TIMING_MODE raise."""
    z, cfg, sd = load(golden_dir)
    x = torch.from_numpy(z["z"])
    T, Tp = x.shape[-1], z["prompt"].shape[-1]
    px = torch.zeros_like(x)
    px[..., :Tp] = torch.from_numpy(z["prompt"])
    style, mu = torch.from_numpy(z["style"]), torch.from_numpy(z["mu"])
    a = (torch.cat([x, x]), torch.cat([px, torch.zeros_like(px)]), torch.from_numpy(z["x_lens"]), torch.from_numpy(z["t"]),
         torch.cat([style, torch.zeros_like(style)]), torch.cat([mu, torch.zeros_like(mu)]))
    taps = {}
    with torch.no_grad():
        plain = S.dit_forward(sd, cfg, *a)
        tapped = S.dit_forward(sd, cfg, *a, taps=taps)
    assert plain.dtype == torch.float32 and torch.equal(plain, tapped)
    np.testing.assert_allclose(plain.numpy(), z["estimator_out"], rtol=0, atol=2e-5)
    H, I, W = cfg.hidden_dim, cfg.intermediate_size, cfg.wavenet_hidden
    want = {"x_in": H, "final_norm": H, "skip_linear": H, "conv1": W, "final_layer": W, "conv2": cfg.in_channels}
    for i in range(cfg.depth):
        want.update({f"dit.{i}.q": H, f"dit.{i}.k": H, f"dit.{i}.ao": H, f"dit.{i}.x_attn": H, f"dit.{i}.swiglu": I, f"dit.{i}.x_ffn": H})
        if i > cfg.depth // 2:
            want[f"dit.{i}.skip_in"] = H
    for i in range(cfg.wavenet_layers):
        want.update({f"wn.{i}.gate": W, f"wn.{i}.x": W, f"wn.{i}.skip": W})
    assert set(taps) == set(want), set(taps) ^ set(want)
    for k, c in want.items():
        assert tuple(taps[k].shape) == (2, T, c) and taps[k].dtype == torch.float32, (k, taps[k].shape)
    assert torch.equal(taps["conv2"].transpose(1, 2), plain)
    sd64 = {k: v.double() for k, v in sd.items()}
    a64 = tuple(t.double() if t.is_floating_point() else t for t in a)
    taps64 = {}
    with torch.no_grad():
        d64 = S.dit_forward(sd64, cfg, *a64, taps=taps64)
    assert d64.dtype == torch.float64 and all(v.dtype == torch.float64 for v in taps64.values())
    assert float((d64 - plain).abs().max()) <= 2e-5
    S.TIMING_MODE = True
    try:
        with torch.no_grad():
            S.dit_forward(sd, cfg, *a)                                   # taps=None: the timing branch still runs
        try:
            S.dit_forward(sd, cfg, *a, taps={})
            raised = False
        except RuntimeError:
            raised = True
    finally:
        S.TIMING_MODE = False
    assert raised


def test_f32_oracle_vs_f64_oracle_on_the_ragged_batch():
    """The f32 oracle's own error: its 3-step CFG solve (rate 0.7) of every utterance of the `tail` batch against the same solve computed in f64
    from the same f32 inputs and weights.  The bound (3e-5 max / 6e-6 rms) is 2x the worst row of the measurement it was set from (per utterance
    max|d| 0.9-1.4e-5, rms 0.8-2.9e-6 at output rms 0.55-1.8), so that a BLAS change does not flip it; with the inputs above this test prints
    max|d| 7.4-8.7e-6 and rms 1.7-2.0e-6 at output rms 1.5-1.8.  The engine's bounds in tests/test_gpu_s2mel_ragged_f64.py (1e-4 / 2e-5) stand
    about 7x over the 1.4e-5 / 2.9e-6 figures."""
    T, Tp, _ = RAGGED["tail"]
    f32, f64 = ragged_solve("tail", 0.7, torch.float32), ragged_solve("tail", 0.7, torch.float64)
    for u in range(len(T)):
        assert f32[u].dtype == torch.float32 and f64[u].dtype == torch.float64 and f64[u].shape == (1, 80, T[u])
        d = f32[u].double() - f64[u]
        print(f"ragged tail utt {u} (T {T[u]}, prompt {Tp[u]}): f32 oracle vs f64 oracle max|d| {float(d.abs().max()):.3e} rms {_rms(d):.3e} "
              f"(output rms {_rms(f64[u]):.3f})")
        assert float(f64[u][..., : Tp[u]].abs().sum()) == 0.0                # (an empty slice for the row without a prompt)
        assert float(d.abs().max()) <= 3e-5 and _rms(d) <= 6e-6
