"""The seeded flow-matching noise on the device: `cfm_noise_kernel` against the numpy restatement (tests/cfm_noise_ref.py), the key as the only
input of a row's noise, the keyed `CFM.inference` against the given-noise path it replaces, and per-row diffusion steps / CFG rates / noise
temperatures through `codes_to_mel` against the CPU oracle chain of every row."""
import numpy as np
import pytest
import torch

from tests.cfm_noise_ref import cfm_noise, cfm_noise_bct
from tests.test_gpu_pipeline import _s2_engines

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENG = {}


def _engines(prec):
    if prec not in _ENG:
        _ENG[prec] = _s2_engines(prec)
    return _ENG[prec]


def _kernel(frames, prompts, seeds, streams, temps, channels, chunks=None):
    """itts_s2mel_noise_forward on the packed rows of sequences of `frames` frames: (sum(frames), channels) f32 on the host, and the row tables"""
    from indextts_amd import _lib
    chunks = [0] * len(frames) if chunks is None else chunks
    seq = np.repeat(np.arange(len(frames), dtype=np.int32), frames)
    t = np.concatenate([np.arange(f, dtype=np.int32) for f in frames])
    keys = [s | (c << 32) for s, c in zip(streams, chunks)]
    as_i64 = lambda vals: torch.tensor([v - (1 << 64) if v >= 1 << 63 else v for v in vals], dtype=torch.int64, device=DEV)
    d = dict(seq=torch.from_numpy(seq).to(DEV), t=torch.from_numpy(t).to(DEV), pl=torch.tensor(prompts, dtype=torch.int32, device=DEV),
             seed=as_i64(seeds), key=as_i64(keys), temp=torch.tensor(temps, dtype=torch.float32, device=DEV))
    n_rows = int(sum(frames))
    x = torch.full((n_rows + 1, channels), float("nan"), device=DEV)                  # one guard row behind the last: must stay untouched
    with _lib.on_device(torch.device(DEV)):
        _lib.check(_lib.lib().itts_s2mel_noise_forward(_lib.ptr(x), _lib.ptr(d["seq"]), _lib.ptr(d["t"]), _lib.ptr(d["pl"]), _lib.ptr(d["seed"]),
                                                       _lib.ptr(d["key"]), _lib.ptr(d["temp"]), len(frames), n_rows, channels,
                                                       _lib.stream_ptr(torch.device(DEV))), "itts_s2mel_noise_forward")
    torch.cuda.synchronize()
    out = x.cpu().numpy()
    assert np.isnan(out[n_rows]).all(), "the kernel wrote behind its last row"
    return out[:n_rows], seq, t


@pytest.mark.parametrize("channels", [80, 6])
def test_kernel_equals_the_restatement(channels):
    frames, prompts, temps = (12, 7, 9), (5, 0, 9), (1.0, 0.5, 0.0)
    seeds, streams = (7, 7, 2 ** 63 + 5), (0, 1, 0)
    got, seq, t = _kernel(frames, prompts, seeds, streams, temps, channels)
    assert got.dtype == np.float32 and got.shape == (sum(frames), channels) and np.isfinite(got).all()
    want = np.zeros_like(got)
    free = np.zeros(got.shape, dtype=bool)                       # elements that are neither prompt frames nor scaled by temperature 0
    for s in range(3):
        rows = np.nonzero((seq == s) & (t >= prompts[s]))[0]
        if rows.size:
            want[rows] = cfm_noise(seeds[s], streams[s], rows.size, channels, temps[s])
            free[rows] = temps[s] != 0.0
    prompt_rows = t < np.array(prompts)[seq]
    assert prompt_rows.sum() == 5 + 0 + 9
    assert (got[prompt_rows] == 0).all() and not np.signbit(got[prompt_rows]).any()            # exactly +0.0f
    assert (got[seq == 2] == 0).all()                                                          # no target frame and temperature 0
    zero_t = _kernel((4,), (1,), (7,), (0,), (0.0,), channels)[0]
    assert (zero_t == 0).all()                                                                 # temperature 0: every row exactly 0
    assert free.sum() == (7 + 7) * channels
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    same = float((got[free] == want[free]).mean())
    print(f"C = {channels}: {int(free.sum())} noise elements, bit-equal {same * 100:.3f} %, max error {float((err[free] / ulp[free]).max()):.2f} ulp")
    assert (err[free] <= ulp[free]).all()
    assert same >= 0.99


def test_the_key_is_everything():
    seed, stream, C_ = 1234, 3, 80
    alone, seq_a, t_a = _kernel((12,), (5,), (seed,), (stream,), (1.0,), C_)
    mixed, seq_b, t_b = _kernel((6, 15, 9), (1, 4, 2), (99, seed + 1, seed), (stream, stream, stream), (1.0, 0.7, 1.0), C_)
    a = torch.from_numpy(alone[t_a >= 5])
    b = torch.from_numpy(mixed[(seq_b == 2) & (t_b >= 2)])
    assert a.shape == b.shape == (7, C_) and torch.equal(a, b)                  # another slot, another prompt length, other rows around it
    assert np.abs(a.numpy().astype(np.float64) - cfm_noise(seed, stream, 7, C_)).max() < 1e-6
    assert not torch.equal(torch.from_numpy(mixed[(seq_b == 1) & (t_b >= 4)][:7]), a)          # another seed: other noise
    c1 = _kernel((12,), (5,), (seed,), (stream,), (1.0,), C_, chunks=(1,))[0]
    assert not np.array_equal(c1[5:], alone[5:]) and np.abs(c1[5:] - alone[5:]).max() > 0.5    # chunk 1 is another stream than chunk 0
    assert np.abs(c1[5:].astype(np.float64) - cfm_noise(seed, stream, 7, C_, chunk=1)).max() < 1e-6


def _cfm_case(gen_seed=62):
    g = torch.Generator().manual_seed(gen_seed)
    total, tp = [17, 13], [6, 3]
    T = max(total)
    mu = torch.randn(2, T, 64, generator=g)
    style = torch.randn(2, 192, generator=g)
    prompt = torch.zeros(2, 80, max(tp))
    for b in range(2):
        prompt[b, :, : tp[b]] = torch.randn(80, tp[b], generator=g) * 0.5 - 1.0
    return total, tp, mu.to(DEV), style.to(DEV), prompt.to(DEV)


def test_keyed_inference_leaves_torch_generator_alone():
    cfm = _engines("fp32")[1].models["cfm"]
    total, tp, mu, style, prompt = _cfm_case()
    torch.manual_seed(3)
    torch.randn(5, device=DEV)
    state = torch.cuda.get_rng_state(0).clone()
    out = cfm.inference(mu, torch.tensor(total), prompt, style, None, 2, inference_cfg_rate=0.7, prompt_lens=tp, frame_lens=total,
                        noise_keys=([5, 6], [0, 1]))
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    assert torch.equal(torch.cuda.get_rng_state(0), state)
    with pytest.raises(ValueError, match="not both"):
        cfm.inference(mu, torch.tensor(total), prompt, style, None, 2, noise=torch.zeros(2, 80, 17), noise_keys=([5, 6], [0, 1]))


@pytest.mark.parametrize("prec", ["fp32", "fp32x3"])
def test_keyed_inference_is_the_given_noise_path(prec):
    cfm = _engines(prec)[1].models["cfm"]
    total, tp, mu, style, prompt = _cfm_case()
    seeds, streams, temps = [7, 2 ** 63 + 5], [0, 4], [1.0, 0.8]
    # the kernel's rows through the solver's own tables, unpacked to the (B, C, T) layout of `noise=`
    tabs, n_tok, _ = cfm._tables(total, torch.tensor(total), 1)
    rows = cfm.noise_rows(tabs["tok_seq"], tabs["tok_t"], tp, seeds, streams, temps, n_tok)
    noise = cfm._unpack_rows(rows, tabs["tok_seq"].long(), tabs["tok_t"].long(), 2, max(total))
    want = cfm_noise_bct(seeds, streams, total, tp, 80, temps)
    assert np.abs(noise.cpu().numpy().astype(np.float64) - want).max() < 1e-6
    kw = dict(inference_cfg_rate=0.7, prompt_lens=tp, frame_lens=total)
    keyed = cfm.inference(mu, torch.tensor(total), prompt, style, None, 4, temperature=temps, noise_keys=(seeds, streams), **kw)
    given = cfm.inference(mu, torch.tensor(total), prompt, style, None, 4, noise=noise, **kw)
    assert bool(torch.isfinite(keyed).all()) and float(keyed[0, :, 6:17].abs().max()) > 0
    assert torch.equal(keyed, given)


def test_per_row_steps_rates_and_temperatures_vs_oracle_chain():
    """3 rows over 2 bundles (prompt lengths 11 and 7), code lengths 9 / 5 / 7, keyed noise; steps (4, 2, 4), CFG rates (0.7, 0.7, 0.0), noise
    temperatures (1.0, 0.8, 1.0): every row equals the CPU oracle chain of that row under its bundle, fed the restated noise at the row's steps
    and rate, at the 2e-4 of test_codes_to_mel_with_per_row_bundles_vs_oracle_chain; and equals the same row alone through `codes_to_mel`."""
    from indextts_amd.s2mel import codes_to_mel
    from oracle import codec_oracle as CO
    from oracle import s2mel_oracle as SO
    c, mm, (cc, rc, sc, csd, rsd, ssd, _) = _engines("fp32")
    cfm = mm.models["cfm"]
    g = torch.Generator().manual_seed(60)
    bundles = []
    for Tp in (11, 7):
        bundles.append(dict(style=torch.randn(1, 192, generator=g).to(DEV), ref_mel=(torch.randn(1, 80, Tp, generator=g) * 0.5 - 1.0).to(DEV),
                            prompt_condition=torch.randn(1, Tp, 64, generator=g).to(DEV)))
    index, lens, tp = [0, 1, 0], [9, 5, 7], [11, 7, 11]
    steps, rates, temps = [4, 2, 4], [0.7, 0.7, 0.0], [1.0, 0.8, 1.0]
    seeds, streams = [21, 22, 21], [0, 0, 1]
    codes = torch.randint(0, 8192, (3, 9), generator=g)
    target = [int(2 * n * 1.72) for n in lens]
    total = [p + t for p, t in zip(tp, target)]
    state = torch.cuda.get_rng_state(0).clone()
    mel, mel_lens = codes_to_mel(c, mm.models, codes.to(DEV), torch.tensor(lens), bundles, 1.0, diffusion_steps=steps, inference_cfg_rate=rates,
                                 bundle_index=index, noise_keys=(seeds, streams), noise_temperature=temps)
    assert torch.equal(torch.cuda.get_rng_state(0), state)
    assert mel_lens.tolist() == target and mel.shape == (3, 80, max(target)) and bool(torch.isfinite(mel).all())
    noise = torch.from_numpy(cfm_noise_bct(seeds, streams, total, tp, 80, temps))
    # the noise part, batch vs alone: the kernel's rows of row b in the batch's tables and in its own
    tabs, n_tok, _ = cfm._tables(total, torch.tensor(total), 1)
    rows = cfm.noise_rows(tabs["tok_seq"], tabs["tok_t"], tp, seeds, streams, temps, n_tok)
    for b, n in enumerate(lens):
        bd, Tp, T = bundles[index[b]], tp[b], total[b]
        with torch.no_grad():
            s = CO.codec_decode(csd, cc, codes[b:b + 1, :n])
            cond, _ = CO.length_regulator(rsd, rc, s, torch.tensor([target[b]]))
            cat = torch.cat([bd["prompt_condition"].cpu(), cond], 1)
            ref = SO.cfm_solve_euler(ssd, sc, noise[b:b + 1, :, :T], torch.tensor([T]), bd["ref_mel"].cpu(), cat, bd["style"].cpu(), steps[b], rates[b])
        err = float((mel[b:b + 1, :, : target[b]].cpu() - ref[:, :, Tp:]).abs().max())
        one, _ = codes_to_mel(c, mm.models, codes[b:b + 1, :n].to(DEV), torch.tensor([n]), bd, 1.0, diffusion_steps=steps[b],
                              inference_cfg_rate=rates[b], noise_keys=([seeds[b]], [streams[b]]), noise_temperature=temps[b])
        own = float((mel[b:b + 1, :, : target[b]] - one).abs().max())
        t1, _, _ = cfm._tables([T], torch.tensor([T]), 1)
        r1 = cfm.noise_rows(t1["tok_seq"], t1["tok_t"], [Tp], [seeds[b]], [streams[b]], [temps[b]], T)
        assert torch.equal(rows[sum(total[:b]): sum(total[:b]) + T], r1)
        print(f"per-row settings, row {b} (bundle {index[b]}, steps {steps[b]}, rate {rates[b]}, temperature {temps[b]}): max|d| vs oracle chain "
              f"{err:.2e}, vs the row alone {own:.2e}")
        assert err <= 2e-4
        assert own <= 2e-4
