"""CPU: the premises of the prompt-side kernel matrix (tests/prompt_matrix.py), which tests/test_gpu_prompt_matrix.py runs on the device.

  reference agreement -- every f64 reference agrees to 1e-12 (relative to its normaliser or its largest value) with an independent statement of
    the same op: torch in f64 (F.layer_norm, F.group_norm + F.mish, F.gelu, F.glu, F.conv1d, F.interpolate, F.avg_pool1d(ceil_mode=True),
    scaled_dot_product_attention with an explicit mask) and the oracles under oracle/ (resample, the FVQ distance, attentive statistics);
  coverage -- the case table reaches every kernel instance and launcher branch the dispatch rules name, and the refusals are ones the rules refuse;
  exact-family premises -- the constants, sums and leftovers the bitwise comparisons rest on;
  mutants -- every named wrong variant of a reference, evaluated in plain f32 in the kernel's place, fails the comparison the GPU test applies on
    at least one launch, while the plain-f32 evaluation of the right definition passes every wide launch with room (it is held to E, the limit is 4 E);
  the VQ exemption -- no case exempts more than 1 % of its rows from the argmax comparison."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import prompt_matrix as PM

F64 = torch.float64
BY_OP = {}
for _c in PM.CASES:
    BY_OP.setdefault(_c.op, []).append(_c)


def _close(got, want, scale=None, tol=1e-12):
    scale = want.abs().max().clamp(min=1e-300) if scale is None else scale
    err = (got - want).abs()
    err = torch.where(err == 0, err, err / scale)                       # (a normaliser of 0, an empty key range, wants the exact result)
    assert float(torch.nan_to_num(err, nan=math.inf).max()) <= tol, float(err.max())


def _each(op, families):
    for c in BY_OP[op]:
        for lch in PM.launches(c, families):
            yield c, lch


# ---- reference agreement ---------------------------------------------------------------------------------------------------------------
def test_layernorm_reference_is_torch_layer_norm():
    for c, lch in _each("layernorm", ("wide",)):
        a = lch.args
        D = a["x"].shape[1]
        y = F.layer_norm(a["x"].double(), (D,), a["g"].double(), a["b"].double(), a["eps"])
        if a["g2"] is not None:
            y = F.layer_norm(y, (D,), a["g2"].double(), a["b2"].double(), a["eps"])
        _close(lch.ref, y, lch.norm)


def test_attention_reference_is_sdpa_per_query():
    for c, lch in _each("attention", ("wide", "uniform")):
        a = lch.args
        nq, H, dq = a["q"].shape
        want = torch.zeros_like(lch.ref)
        for m in range(nq):
            ks, kl = int(a["kstart"][m]), int(a["klen"][m])
            if kl == 0:
                continue
            k, v = a["k"][ks:ks + kl].double().transpose(0, 1), a["v"][ks:ks + kl].double().transpose(0, 1)      # [H][kl][d]
            q = a["q"][m].double()[:, None, :]                                                                     # [H][1][dq]
            bias = None
            if a.get("emb") is not None:
                r = (torch.arange(kl) - int(a["qpos"][m])).clamp(-a["left"], a["right"]) + a["left"]
                bias = (a["q"][m].double() @ a["emb"].double()[r].T)[:, None, :] * a["scale"]                      # [H][1][kl]
            want[m] = F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=a["scale"])[:, 0, :]
        _close(lch.ref, want, lch.norm if lch.norm is not None else None)


def test_pointwise_references_are_torch():
    for op in ("gelu", "glu", "act", "gate", "scale_residual", "affine"):
        for c, lch in _each(op, ("wide", "exact")):
            a = lch.args
            x = a["x"].double()
            mode = a.get("mode", 0)
            if op == "gelu":
                want = F.gelu(x)
            elif op == "glu":
                want = F.glu(x, -1) if mode == 0 else x[:, :a["C"]] * F.gelu(x[:, a["C"]:])
            elif op == "act":
                want = (F.relu, F.silu, torch.tanh)[mode](x)
            elif op == "gate":
                want = x * torch.sigmoid(a["g"].double())
            elif op == "scale_residual":
                want = torch.addcmul(x, a["gamma"].double()[None, :], a["y"].double())
            else:
                want = torch.addcmul(a["shift"].double()[None, :], x[:, :a["C"]], a["scale"].double()[None, :])
                want = F.relu(want) if a["relu"] else want
            _close(lch.ref, want, lch.norm if lch.norm is not None else None)


def test_dwconv_reference_is_conv1d_per_sequence():
    for c, lch in _each("dwconv", ("wide",)):
        a = lch.args
        k, C = a["k"], a["x"].shape[1]
        start = 0
        for s, T in enumerate(a["seq_T"].tolist()):
            if T and bool(lch.valid[start].all()):
                x = a["x"][start:start + T].double().T[None]                                                       # [1][C][T]
                pad = (k - 1, 0) if a["causal"] else ((k - 1) // 2, (k - 1) // 2)
                y = F.conv1d(F.pad(x, pad), a["w"].double()[:, None, :], a["b"].double() if a["b"] is not None else None, groups=C)[0].T
                _close(lch.ref[start:start + T], y, lch.norm[start:start + T])
            start += T


def test_gather_reference_is_interpolate_then_unfold():
    for c, lch in _each("gather_conv", ("exact",)):
        a = lch.args
        k, C = a["k"], a["C"]
        row = 0
        for s in range(a["src_T"].numel()):
            Ts, Td, st = int(a["src_T"][s]), int(a["dst_T"][s]), int(a["src_start"][s])
            x = a["x"][st:st + Ts].T[None]                                                                         # [1][C][Ts] f32: torch's own nearest rule
            up = F.interpolate(x, size=Td, mode="nearest") if Ts != Td else x
            col = F.pad(up, ((k - 1) // 2, (k - 1) // 2)).unfold(2, k, 1)[0].permute(1, 2, 0).reshape(Td, k * C)   # [Td][k][C]
            assert torch.equal(lch.ref[row:row + Td], col.double()), (Ts, Td)
            row += Td


def test_groupnorm_mish_reference_is_torch():
    for c, lch in _each("groupnorm_mish", ("wide",)):
        a = lch.args
        for s, T in zip(a["seq_start"].tolist(), a["seq_T"].tolist()):
            if T:
                x = a["x"][s:s + T].double().T[None]
                y = F.mish(F.group_norm(x, 1, a["gamma"].double(), a["beta"].double(), a["eps"]))[0].T
                _close(lch.ref[s:s + T], y, lch.norm[s:s + T])
        assert bool(torch.isnan(lch.ref[~lch.valid]).all()) and not bool(torch.isnan(lch.ref[lch.valid]).any())


def test_l2norm_colnorm_references_are_torch():
    for c, lch in _each("l2norm", ("wide",)):
        a = lch.args
        _close(lch.ref, F.normalize(a["x"].double(), dim=-1) * a["scale"] * a["gamma"].double(), lch.norm)
        assert bool((lch.ref[3] == 0).all())
    for c, lch in _each("colnorm", ("wide",)):
        a = lch.args
        x = a["x"].double()
        want = x - x.mean(0)
        if a["mode"] == 1:
            want = want / torch.sqrt(x.var(0, correction=a["ddof"]) + a["eps"]) if x.shape[0] > a["ddof"] else want
        C = x.shape[1]
        _close(lch.ref[:, :C], want, lch.norm[:, :C])


def test_pool_references_are_torch_and_the_oracle():
    from oracle import ecapa_oracle
    for c, lch in _each("ctxpool", ("wide",)):
        a = lch.args
        x = a["x"].double().T[None]                                                                                # [1][C][n]
        n, seg = x.shape[2], a["seg_len"]
        pooled = F.avg_pool1d(x, kernel_size=seg, stride=seg, ceil_mode=True)
        want = x.mean(-1, keepdim=True) + pooled.repeat_interleave(seg, dim=2)[:, :, :n]
        _close(lch.ref, want[0].T, lch.norm)
    for c, lch in _each("statspool", ("wide",)):
        x = lch.args["x"].double()
        _close(lch.ref, torch.stack([x.mean(0), x.var(0, correction=1)]), lch.norm)
    for c, lch in _each("attnstats", ("wide",)):
        a = lch.args
        x = a["x"].double().T[None]                                                                                # [1][C][n]
        n = x.shape[2]
        w = torch.softmax(a["logit"].double().T[None], dim=2) if a["logit"] is not None else torch.full_like(x, 1.0 / n)
        mean, std = ecapa_oracle._stats(x, w, a["eps"])
        _close(lch.ref, torch.stack([mean[0], std[0] ** 2]), lch.norm, tol=1e-11)


def test_vq_references_are_the_oracle_statements():
    for c, lch in _each("vq_project", ("wide",)):
        a = lch.args
        want = F.conv1d(F.embedding(a["codes"], a["codebook"].double()).T[None], a["w"].double()[:, :, None], a["bias"].double())[0].T
        _close(lch.ref, want, lch.norm)
    for c, lch in _each("vq_search", ("index",)):
        a = lch.args
        # FVQ.forward's own expression (factorized_vector_quantize.py:99-118 as oracle/codec_oracle.py states it): -(|e|^2 - 2 e c^T + |c|^2), max(1)
        z = F.conv1d(a["h"].double().T[None], a["w_in"].double()[:, :, None], a["b_in"].double())[0].T
        e, cb = F.normalize(z), F.normalize(a["cb_norm"].double())
        dist = e.pow(2).sum(1, keepdim=True) - 2 * e @ cb.t() + cb.pow(2).sum(1, keepdim=True).t()
        held = lch.norm > PM.VQ_MARGIN
        assert torch.equal((-dist).max(1)[1][held], lch.ref.long()[held])


def test_resample_reference_is_the_oracle():
    from oracle import audio_oracle
    for c in BY_OP["resample"]:
        p = PM.P(c)
        kern, width = PM.resample_table(p["orig"], p["new"])
        ok, ow, _, _ = audio_oracle.sinc_resample_kernel(p["orig"], p["new"])
        assert ow == width and float((ok.double() - kern.double()).abs().max()) <= 2.0 ** -23                       # two roundings of the same f64 table
        for lch in PM.launches(c, ("wide",)):
            a = lch.args
            L_in, L_out = a["L_in"], a["L_out"]
            x = F.pad(a["x"][:, :L_in].double(), (width, 3 * width + 2 * p["orig"]))                              # zeros enough for the largest L_out
            y = F.conv1d(x[:, None], kern.double()[:, None], stride=p["orig"]).transpose(1, 2).reshape(2, -1)
            _close(lch.ref[:, :L_out], y[:, :L_out], lch.norm[:, :L_out])


def test_fbank_reference_is_torch_fft_stft_and_the_kaldi_oracle():
    from oracle import audio_oracle
    for c, lch in _each("fbank", ("wide",)):
        a = lch.args
        n, FL, hop, N, pad, M = a["n_samples"], a["FL"], a["hop"], a["n_fft"], a["pad"], a["n_mels"]
        frames = PM.fbank_frames(FL, hop, pad, n)
        assert int(lch.valid.sum()) == 2 * frames * M
        if frames == 0:
            continue
        w = a["wave"][:, :n].double() * a["scale"]
        padded = F.pad(w[:, None], (pad, pad), mode="reflect")[:, 0] if pad else w
        fr = padded.unfold(-1, FL, hop)                                                                            # [B][frames][FL]
        assert fr.shape[1] == frames
        if a["remove_dc"]:
            fr = fr - fr.mean(-1, keepdim=True)
        if a["preemph"]:
            fr = fr - a["preemph"] * F.pad(fr, (1, 0), mode="replicate")[..., :-1]
        X = torch.fft.fft(fr * a["window"].double(), n=N)[..., :N // 2 + 1]                                        # the full complex transform
        Pw = X.abs() ** 2 if a["power"] == 2 else (X.abs() ** 2 + a["mag_eps"]).sqrt()
        want = (Pw @ a["mel"].double().T).clamp(min=a["floor"])
        want = want.log() if a["take_log"] else want
        ld = a["ld_out"]
        got = (lch.ref[:, :frames * ld].view(2, frames, ld)[:, :, :M] if a["layout"] == 0 else lch.ref[:, :M * ld].view(2, M, ld)[:, :, :frames].transpose(1, 2))
        nrm = (lch.norm[:, :frames * ld].view(2, frames, ld)[:, :, :M] if a["layout"] == 0 else lch.norm[:, :M * ld].view(2, M, ld)[:, :, :frames].transpose(1, 2))
        _close(got, want, nrm, tol=1e-11)
        if c.name == "mel":                                            # torch.stft over the reflect-padded waveform, as mel_spectrogram calls it
            spec = torch.stft(padded, N, hop_length=hop, win_length=FL, window=a["window"].double(), center=False, return_complex=True)
            mel = (a["mel"].double() @ (spec.abs() ** 2 + a["mag_eps"]).sqrt()).clamp(min=a["floor"])              # [B][M][frames]
            _close(got.transpose(1, 2), mel.log() if a["take_log"] else mel, nrm.transpose(1, 2), tol=1e-11)
        if c.name == "kaldi" and a["take_log"]:                        # the oracle builds its own Povey window in f64, the engine's table is f32
            for b in range(2):                                         # (2^-25 of each sample): 1e-6 of the normaliser
                _close(got[b], audio_oracle.kaldi_fbank(w[b], dtype=torch.float64), nrm[b], tol=1e-6)


# ---- coverage --------------------------------------------------------------------------------------------------------------------------
def test_fbank_table_covers_the_listed_shapes():
    ps = [PM.P(c) for c in BY_OP["fbank"]]
    assert {p["n_fft"] for p in ps} == {64, 512, 1024, 2048} and {p["n_mels"] for p in ps} == {1, 3, 4, 5, 80, 100} and {p["hop"] for p in ps} >= {1, 160, 256}
    assert {(p["n_fft"], p["FL"]) for p in ps} >= {(512, 400), (64, 2), (64, 64)}
    assert {p["layout"] for p in ps} == {0, 1} and {p["power"] for p in ps} == {1, 2} and {p["remove_dc"] for p in ps} == {0, 1}
    frames = {PM.fbank_frames(p["FL"], p["hop"], p["pad"], n) for p in ps if p["pad"] == 0 for n in p["n_samples"]}
    assert {0, 1} < frames
    for p in ps:
        if p["pad"]:
            assert p["pad"] == (p["n_fft"] - p["hop"]) // 2 and p["pad"] + 1 in p["n_samples"] and all(n > p["pad"] for n in p["n_samples"])
        for n in p["n_samples"]:                                        # every sample index a frame reads reflects once at most
            t = PM.fbank_frames(p["FL"], p["hop"], p["pad"], n)
            assert t == 0 or (t - 1) * p["hop"] - p["pad"] + p["FL"] - 1 <= 2 * (n - 1)
def test_every_instance_and_branch_has_a_case():
    hit = set()
    for c in PM.CASES:
        inst = PM.instances_of(c)
        assert inst and all(i in PM.ALL_INSTANCES for i in inst), (PM.case_id(c), inst)
        hit.update(inst)
    assert sorted(set(PM.ALL_INSTANCES) - hit) == []
    assert len(set(map(PM.case_id, PM.CASES))) == len(PM.CASES)


def test_layernorm_table_is_the_dispatch_rule():
    assert len(PM.LN_NE_ALL) == 14 and len(PM.LN_NV) == 7 and len(PM.LN_NE) == 7
    Ds = {PM.P(c)["D"] for c in BY_OP["layernorm"]}
    assert {256 * nv for nv in PM.LN_NV} | {64 * ne for ne in PM.LN_NE} | set(PM.LN_GENERIC_D) == Ds
    for ne in PM.LN_NE_ALL:                                             # an instantiated small width that is a multiple of 256 is never launched
        assert (PM.ln_instance(64 * ne, 4, False) or "").startswith("ln_small_kernel" if ne in PM.LN_NE else "ln_kernel")
    assert PM.ln_instance(1024, 256, True) == "ln_kernel<4>/wpb1" and PM.ln_instance(1024, 257, True) == "ln_kernel<4>/wpb4"
    for D, second in PM.LN_REFUSALS:
        assert PM.ln_instance(D, 4, second) is None
    rows = {lch.args["x"].shape[0] for lch in PM.launches(BY_OP["layernorm"][0])}
    assert rows == set(PM.LN_ROWS) and {r % 4 for r in rows} == {0, 1, 3}


def test_attention_table_covers_the_listed_shapes():
    ps = [PM.P(c) for c in BY_OP["attention"]]
    assert {p["dq"] for p in ps} == {4, 24, 64, 128, 256} and {p["dv"] for p in ps} == {4, 20, 64, 68, 128} and {p["H"] for p in ps} == {1, 3}
    assert {p["rel"] for p in ps} == {None, (0, 0), (9, 4), (64, 8), (255, 256)} and 255 + 256 + 1 == PM.ATTN_REL_MAX
    for c in BY_OP["attention"]:
        kstart, klen, qpos, nk, used = PM.attn_geometry(c)
        assert set(PM.ATTN_KLENS) <= set(klen.tolist()) and int(kstart.min()) > 0
        assert bool((kstart[1:] != kstart[:-1]).all())                  # consecutive queries belong to different sequences
        assert bool(((kstart + klen) <= nk).all()) and bool((qpos >= 0).all()) and bool((qpos < klen.clamp(min=1)).all())
        rel = PM.P(c)["rel"]
        if rel is not None:                                             # both clamps are passed, and some query has its whole range on one side
            left, right = rel
            far_r, far_l = (klen - 1 - qpos).max(), qpos.max()
            assert int(far_r) > right and int(far_l) > left
            assert bool(((qpos == 0) & (klen > 1)).any()) and bool(((qpos == klen - 1) & (klen > 1)).any())
    for r in PM.ATTN_REFUSALS:
        assert r["dv"] > 128 or r["dq"] % 4 or r.get("left", 0) + r.get("right", 0) + 1 > PM.ATTN_REL_MAX


def test_every_index_of_every_table_is_in_range():
    for c in PM.CASES:
        for lch in PM.launches(c):
            a = lch.args
            if c.op in ("dwconv", "gather_conv"):
                n = a["tok_seq"].numel()
                T = (a["seq_T"] if c.op == "dwconv" else a["dst_T"]).long()
                assert bool((a["tok_t"].long() < T[a["tok_seq"].long()]).all()) and bool((a["tok_t"] >= 0).all()) and n == int(T.sum())
            if c.op == "gather_conv":
                assert bool((a["src_start"] >= 0).all()) and int((a["src_start"] + a["src_T"]).max()) <= a["x"].shape[0]
            if c.op == "groupnorm_mish":
                assert int((a["seq_start"] + a["seq_T"]).max()) <= a["x"].shape[0] and int(a["seq_start"].min()) >= 0
            if c.op == "vq_project":
                assert int(a["codes"].min()) == 0 and int(a["codes"].max()) == a["K"] - 1
            if c.op == "resample":
                assert 1 <= a["L_out"] <= PM.resample_full(a["L_in"], a["orig"], a["new"]) and a["x_stride"] >= a["L_in"] and a["y_stride"] >= a["L_out"]


# ---- exact-family premises -------------------------------------------------------------------------------------------------------------
def test_layernorm_constants_make_the_f32_mean_exact():
    for c in BY_OP["layernorm"]:
        D = PM.P(c)["D"]
        cst = np.float32(PM.ln_constant(D))
        total = np.float32(cst * np.float32(D))
        assert float(total) == float(cst) * D and abs(float(total)) < 2 ** 24            # every partial sum of the row is a multiple of 1/4 under 2^24
        assert total * (np.float32(1.0) / np.float32(D)) == cst


def test_exact_operands_have_exact_partial_sums():
    """Every term is a multiple of 1/16 and the sum of the magnitudes stays under 2^20: any f32 summation order is exact."""
    for op in ("dwconv", "vq_project", "scale_residual", "affine"):
        for c, lch in _each(op, ("exact",)):
            a = lch.args
            for key in ("x", "w", "b", "y", "gamma", "scale", "shift", "codebook", "bias"):
                t = a.get(key)
                if torch.is_tensor(t) and t.is_floating_point():
                    t = t[~torch.isnan(t)]
                    assert bool(((t * 4) == (t * 4).round()).all()) and float(t.abs().max()) <= 8
            _, mag = PM.OPS[op].evaluate(dict(a, x=torch.nan_to_num(a["x"], nan=0.0)) if "x" in a else a, F64)
            assert float(mag.max()) < 2 ** 20 / 16
            assert torch.equal(lch.ref.float().double()[lch.valid], lch.ref[lch.valid])


def test_onehot_leftovers_are_under_half_an_ulp():
    assert math.exp(-40.0) * (600 - 1) * 255.0 < 2.0 ** -25
    for c in BY_OP["attention"]:
        assert PM.onehot_leftover(c) < 2.0 ** -25
        for lch in PM.launches(c, ("exact",)):
            full = PM.evaluate(c, lch, F64)                            # the definition in f64, rounded once to f32, is the V row
            assert PM.check(c, lch, full) == []
    for c, lch in _each("attnstats", ("exact",)):
        n = lch.args["x"].shape[0]
        assert math.exp(-80.0) * n * 255.0 < 2.0 ** -25 and math.exp(-80.0) * n * 510.0 ** 2 < 1e-12
        assert float(lch.ref[0].abs().min()) >= 1


def test_resample_impulses_return_single_taps():
    for c, lch in _each("resample", ("exact",)):
        a = lch.args
        hits = (a["x"][:, :a["L_in"]] != 0).sum(1)
        assert hits.tolist() == [1, 1]
        got = lch.ref[lch.valid]
        taps = torch.cat([a["kernel"].double().flatten(), -2 * a["kernel"].double().flatten(), torch.zeros(1, dtype=F64)])
        assert bool(torch.isin(got, taps).all())


def test_vq_tie_scores_are_exact_and_tied():
    multi = 0
    for c, lch in _each("vq_search", ("exact",)):
        a = lch.args
        s64, s32 = PM.vq_search_scores(a, F64), PM.vq_search_scores(a, torch.float32)
        assert torch.equal(s64, s32.double()) and set(s64.unique().tolist()) <= {0.0, -2.0, -4.0}
        ties = (s64 == s64.max(1, keepdim=True).values).sum(1)
        multi += int((ties > 1).sum())
        first = torch.tensor([int((row == row.max()).nonzero()[0]) for row in s64])
        assert torch.equal(first, lch.ref.long())
    assert multi > 20
    wins = {int(i) for c, lch in _each("vq_search", ("exact",)) for i in lch.ref.tolist()}
    assert {0, 255, 256, 8191, 63, 44, 1} <= wins


def test_gather_pairs_include_f32_floor_disagreements():
    found = PM.floor_disagreeing_pairs()
    assert len(found) >= 2
    for Ts, Td in found:
        u = np.arange(Td)
        assert (PM.nearest_index(u, Ts, Td) != PM.nearest_index(u, Ts, Td, exact=True)).any()
    for c, lch in _each("gather_conv", ("exact",)):
        pairs = set(zip(lch.args["src_T"].tolist(), lch.args["dst_T"].tolist()))
        assert set(PM.GATHER_PAIRS) | set(found) == pairs


# ---- mutants ---------------------------------------------------------------------------------------------------------------------------
def test_plain_f32_passes_every_wide_launch_at_E():
    for c in PM.CASES:
        for lch in PM.launches(c, ("wide",)):
            st = {}
            assert PM.check(c, lch, PM.evaluate(c, lch, torch.float32), st) == []
            assert st["ratio"] <= 1 / PM.MARGIN + 1e-12
    for op in PM.OPS:
        if any(True for c in BY_OP[op] for _ in PM.launches(c, ("wide",))):
            assert 2.0 ** -26 < PM.baseline_E(op) < 1e-5, (op, PM.baseline_E(op))


@pytest.mark.parametrize("mutant", sorted(PM.MUTANTS))
def test_mutant_is_caught(mutant):
    caught = []
    for c in BY_OP[PM.MUTANTS[mutant]]:
        for lch in PM.launches(c):
            out = PM.evaluate(c, lch, torch.float32, mutant)
            if PM.check(c, lch, out):
                caught.append(f"{PM.case_id(c)}/{lch.label}")
    assert caught, f"no launch notices {mutant}"
    print(mutant, "caught by", len(caught), "launches, e.g.", caught[:3])


# ---- the VQ exemption ------------------------------------------------------------------------------------------------------------------
def test_vq_exempt_share_is_under_one_percent():
    seen = 0
    for c, lch in _each("vq_search", ("index",)):
        share = float((lch.norm <= PM.VQ_MARGIN).float().mean())
        print(PM.case_id(c), "exempt share", share)
        assert share <= PM.VQ_EXEMPT_SHARE
        seen += 1
    assert seen == 5
    big = [lch for c, lch in _each("vq_search", ("index",)) if PM.P(c)["K"] in (8192, 257)]
    assert all(float((lch.norm <= PM.VQ_MARGIN).float().sum()) == 0 for lch in big)
