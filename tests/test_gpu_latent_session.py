"""GPU tests of the teacher-forced latent SESSION (`itts_gpt_latent_open / _append / _close`, `UnifiedVoice.latent_session`) and of the
IndexTTS-2 streaming pipeline built on it (`indextts_amd.infer_v2.IndexTTS2.infer_stream`).

The session is the one-shot latent pass (`itts_gpt_forward_latent`, model_v2.py:596-646) with its KV cache kept: the pass is causal and
unmasked, so appending a row's codes piece by piece must give the latents the finished utterance gets.  Bars:
  * f32 engine vs the reference-minted fixtures / the CPU oracle: atol 5e-5, the bar tests/test_gpu_gpt.py holds the one-shot pass to;
  * bf16 engine: the contract and bounds of `test_bf16_latents_and_logits_vs_reference_fixture` (0.02 vs the CPU restatement of the bf16
    contract, 0.03 vs the reference's fp32 latents).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ATOL = 5e-5
BF16_LATENT_VS_CONTRACT = 0.02           # tests/test_gpu_gpt.py:527-528
BF16_LATENT_VS_F32_SMALL = 0.03


def _cfg(z):
    c = z["cfg"]
    return G.GPTConfig(layers=int(c[0]), model_dim=int(c[1]), heads=int(c[2]), max_text_tokens=int(c[3]), max_mel_tokens=int(c[4]),
                       number_text_tokens=int(c[5]))


def _case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name))
    cfg = _cfg(z)
    sd = dict(G.synth_weights(cfg, seed=int(z["seed"])))
    sd["mel_head.bias"][cfg.stop_mel_token] += float(z["eos_bias"])
    return z, cfg, sd


def _engine(cfg, sd, precision="fp32", campplus=True):
    from indextts_amd import gpt
    kw = dict(spk_cond_mode="campplus") if campplus else {}
    m = gpt.UnifiedVoice(layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, max_text_tokens=cfg.max_text_tokens,
                         max_mel_tokens=cfg.max_mel_tokens, number_text_tokens=cfg.number_text_tokens, precision=precision, device=DEV, **kw)
    m.load_state_dict(sd)
    return m


def _stop_padded(codes, lens, stop):
    codes = codes.clone()
    for b in range(codes.shape[0]):
        codes[b, int(lens[b]):] = stop
    return codes


def _append_in_pieces(sess, codes, pieces):
    out, at = [], 0
    for n in pieces:
        n = codes.shape[1] - at if n is None else n
        out.append(sess.append(codes[:, at:at + n]))
        at += n
    assert at == codes.shape[1] and sess.appended == at
    return torch.cat(out, dim=1).cpu()


def _fixture_inputs(m, z, v2):
    B = z["text"].shape[0]
    text, tl = torch.from_numpy(z["text"]), torch.from_numpy(z["text_lens"])
    if v2:
        conds = m.latent_conds(torch.from_numpy(z["spk_latent"]).repeat(B, 1, 1), torch.from_numpy(z["emo_vec"]).repeat(B, 1),
                               torch.zeros(B, dtype=torch.long))
    else:
        conds = m.latent_conds(m.conds_latent(torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"]))[1].repeat(B, 1, 1),
                               torch.from_numpy(z["emo_vec"]).repeat(B, 1))
    return conds, text, tl


# ---- 1. the reference fixtures, equal prefix lengths (as minted), uneven pieces --------------------------------------------------------
@pytest.mark.parametrize("name,v2", [("gpt_latent.npz", False), ("gpt_v2.npz", True)])
@pytest.mark.parametrize("pieces", [(1, 5, 3, None), (None,)])
def test_session_equals_reference_fixture(golden_dir, name, v2, pieces):
    z, cfg, sd = _case(golden_dir, name)
    if v2:
        sd["speed_emb.weight"] = torch.from_numpy(z["speed_emb"])
    m = _engine(cfg, sd, "fp32", campplus=not v2)
    conds, text, tl = _fixture_inputs(m, z, v2)
    if not v2:          # the campplus conds of `forward`: (spk + emo | 0 | 0) -- the block the one-shot test hands to forward_latent
        ref_conds = m.conds_latent(torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"]))[0].repeat(text.shape[0], 1, 1)
        assert torch.equal(conds.cpu(), ref_conds.cpu())
    # the fixture was minted on the padded batch: every row's text runs to the full width, stop text ids from its own length on
    L = text.shape[1]
    text_p = torch.where(torch.arange(L)[None] >= tl[:, None], torch.full_like(text, m.stop_text_token), text)
    codes = _stop_padded(torch.from_numpy(z["mel_codes"]), z["mel_lens"], cfg.stop_mel_token)
    with m.latent_session(conds, text_p, torch.full((text.shape[0],), L), max_codes=codes.shape[1], max_append=codes.shape[1]) as sess:
        assert len(set(sess.prefix_lens)) == 1
        lat = _append_in_pieces(sess, codes.to(DEV), pieces).numpy()
    err = float(np.abs(lat - z["latent"]).max())
    print(f"latent session vs {name} ({'pieces ' + str(pieces)}): max|d| {err:.2e} (bound {ATOL})")
    assert lat.shape == z["latent"].shape
    np.testing.assert_allclose(lat, z["latent"], rtol=0, atol=ATOL)


# ---- 2. ragged prefixes: every row equals the oracle's pass over that row ALONE ------------------------------------------------------
def _ragged(golden_dir, precision, opts):
    from indextts_amd import _lib
    z, cfg, sd = _case(golden_dir, "gpt_latent.npz")
    m = _engine(cfg, sd, precision)
    conds, text, tl = _fixture_inputs(m, z, False)
    assert len(set(tl.tolist())) == 3                                    # 10 / 7 / 4 text tokens
    codes = _stop_padded(torch.from_numpy(z["mel_codes"]), z["mel_lens"], cfg.stop_mel_token)
    n = codes.shape[1]
    with _lib.option_scope(**opts):
        with m.latent_session(conds, text, tl, max_codes=n + 3, max_append=8) as sess:
            assert sess.prefix_lens == [conds.shape[1] + int(t) + 2 for t in tl]
            lat = _append_in_pieces(sess, codes.to(DEV), (1, 5, 3, 8, None))
        one = m.forward_latent(conds, text, tl, codes, torch.from_numpy(z["mel_lens"])).cpu()       # the padded one-shot pass: information
    return z, cfg, sd, conds.cpu(), text, tl, codes, lat, one


@pytest.mark.parametrize("opts", [{}, {"prefill_attn": 1}], ids=["default_attn", "mfma_attn"])
def test_ragged_session_rows_equal_oracle_alone_f32(golden_dir, opts):
    z, cfg, sd, conds, text, tl, codes, lat, one = _ragged(golden_dir, "fp32", opts)
    n = codes.shape[1]
    for b in range(text.shape[0]):
        t = int(tl[b])
        with torch.no_grad():
            ref = G.forward_latent(sd, cfg, conds[b:b + 1], text[b:b + 1, :t], torch.tensor([t]), codes[b:b + 1], torch.tensor([n]))
        err = float((lat[b] - ref[0]).abs().max())
        print(f"ragged session ({opts or 'default attention'}), row {b} ({t} text tokens) vs the oracle on the row alone: max|d| {err:.2e} "
              f"(bound {ATOL}); vs the engine's padded one-shot pass {float((lat[b] - one[b]).abs().max()):.2e} (information)")
        assert err <= ATOL


def test_ragged_session_bf16_vs_contract(golden_dir):
    z, cfg, sd, conds, text, tl, codes, lat, one = _ragged(golden_dir, "bf16", {})
    n = codes.shape[1]
    for b in range(text.shape[0]):
        t = int(tl[b])
        with torch.no_grad(), G.numerics("bf16"):
            ref = G.forward_latent(G.bf16_weights(sd), cfg, conds[b:b + 1], text[b:b + 1, :t], torch.tensor([t]), codes[b:b + 1], torch.tensor([n]))
        err = float((lat[b] - ref[0]).abs().max())
        print(f"ragged bf16 session, row {b} ({t} text tokens) vs the bf16 contract on the row alone: max|d| {err:.2e} "
              f"(bound {BF16_LATENT_VS_CONTRACT}); vs the engine's padded one-shot pass {float((lat[b] - one[b]).abs().max()):.2e} (information)")
        assert err <= BF16_LATENT_VS_CONTRACT


def test_bf16_session_on_the_bf16_fixture(golden_dir):
    """the inputs and both bounds of test_bf16_latents_and_logits_vs_reference_fixture, through the session in uneven pieces"""
    z, cfg, sd = _case(golden_dir, "gpt_bf16.npz")
    m = _engine(cfg, sd, "bf16")
    conds, text, tl = _fixture_inputs(m, z, False)
    codes, ml = torch.from_numpy(z["mel_codes"]), torch.from_numpy(z["mel_lens"])
    with m.latent_session(conds, text, tl, max_codes=codes.shape[1], max_append=16) as sess:
        lat = _append_in_pieces(sess, _stop_padded(codes, ml, cfg.stop_mel_token).to(DEV), (1, 5, 3, None))
    with torch.no_grad(), G.numerics("bf16"):
        contract = G.forward_latent(G.bf16_weights(sd), cfg, conds.cpu(), text, tl, codes, ml)
    e_contract = float((lat - contract).abs().max())
    e_f32 = float((lat - torch.from_numpy(z["latent_f32"])).abs().max())
    print(f"bf16 session on gpt_bf16.npz: vs contract {e_contract:.2e} (bound {BF16_LATENT_VS_CONTRACT}), vs reference fp32 {e_f32:.4f} "
          f"(bound {BF16_LATENT_VS_F32_SMALL})")
    assert e_contract <= BF16_LATENT_VS_CONTRACT and e_f32 <= BF16_LATENT_VS_F32_SMALL


# ---- 3. beside a suspended decode loop ---------------------------------------------------------------------------------------------------
def test_session_beside_a_suspended_decode_loop(golden_dir):
    z, cfg, sd = _case(golden_dir, "gpt_greedy.npz")
    m = _engine(cfg, sd, "fp32")
    m.post_init_gpt2_config(kv_cache=bool(z["kv_cache"]))
    text, langs = torch.from_numpy(z["text"]).to(DEV), torch.from_numpy(z["langs"]).to(DEV)
    style, emo = torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"])
    B, max_gen = text.shape[0], int(z["max_gen"])
    kw = dict(langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=max_gen, num_beams=1, repetition_penalty=10.0, do_sample=False)
    full, _ = m.inference_speech(None, text, **kw)
    full = full.cpu()
    assert np.array_equal(full.numpy(), z["codes"])                      # the reference's ids, no session anywhere
    tl = (text != m.stop_text_token).sum(1).cpu()
    conds = m.latent_conds(m.conds_latent(style, emo)[1].repeat(B, 1, 1), emo.repeat(B, 1))
    chunk, ovl = 8, 3
    emb, mask, max_new, hf = m.inference_speech_stream(None, text, chunk, ovl, **kw)
    got = torch.full((B, max_gen), cfg.stop_mel_token, dtype=torch.int64)
    lats, appended, k = [], 0, 0
    sess = m.latent_session(conds, text.cpu(), tl, max_codes=max_gen, max_append=chunk)
    for codes, is_last, done, lens in m.generate_chunks(emb, mask, max_new, chunk, ovl, **hf):
        pos = k * (chunk - ovl)
        got[:, pos:pos + codes.shape[1]] = codes.cpu()
        new = codes[:, appended - pos:]                                  # the decode loop is suspended here: append between two chunks
        if new.shape[1]:
            lats.append(sess.append(new).cpu())
            appended += new.shape[1]
        k += 1
    sess.close()
    assert k >= 2
    assert torch.equal(got[:, :full.shape[1]], full), "a latent session changed the ids of the decode loop it ran beside"
    lat = torch.cat(lats, dim=1)
    n = lat.shape[1]
    ref = m.forward_latent(conds, text.cpu(), tl, got[:, :n], torch.full((B,), n)).cpu()       # padded one-shot pass over the final codes ...
    # ... which sees each row's text padding; the session runs rows unpadded, so compare per row, the one-shot pass on the row alone
    for b in range(B):
        t = int(tl[b])
        ref_b = m.forward_latent(conds[b:b + 1], text[b:b + 1, :t].cpu(), torch.tensor([t]), got[b:b + 1, :n], torch.tensor([n])).cpu()
        err = float((lat[b] - ref_b[0]).abs().max())
        print(f"session beside the decode loop, row {b}: vs forward_latent on the final codes {err:.2e} (bound {ATOL}); padded batch pass "
              f"{float((lat[b] - ref[b]).abs().max()):.2e} (information)")
        assert err <= ATOL


# ---- 5. the IndexTTS-2 pipeline ----------------------------------------------------------------------------------------------------------
def test_v2_infer_stream(tmp_path):
    import json
    import yaml
    from oracle import bigvgan_oracle as BO
    from indextts_amd.infer_v2 import IndexTTS2 as IndexTTS2V2
    from tests.test_gpu_pipeline import _FrontendV2, _v2_checkpoint_pieces
    gcfg, cfg, sd, width, D = _v2_checkpoint_pieces()
    h = dict(BO.V2_HPARAMS, upsample_initial_channel=512)
    d = tmp_path / "ckpt"
    (d / "hf_cache" / "bigvgan").mkdir(parents=True)
    (d / "config.yaml").write_text(yaml.safe_dump({"gpt": gcfg, "gpt_checkpoint": "gpt.pth", "version": 2.0}))
    torch.save({"model": sd}, d / "gpt.pth")
    (d / "hf_cache" / "bigvgan" / "config.json").write_text(json.dumps(h))
    torch.save({"generator": BO.synth_weights(h, seed=43)}, d / "hf_cache" / "bigvgan" / "bigvgan_generator.pt")
    fe = _FrontendV2(D, width, device=DEV)
    tts = IndexTTS2V2(cfg_path=str(d / "config.yaml"), model_dir=str(d), use_fp16=False, device=DEV, frontend=fe)
    texts = ["a first streamed sentence", "short", "another one of middle size"]
    chunk, ovl = 8, 2
    pieces, done_at, n = [[] for _ in texts], [None] * len(texts), 0
    for sr, audio, done in tts.infer_stream("spk.wav", texts, top_k=1, max_mel_tokens=30, chunk_size=chunk, overlap_size=ovl):
        assert sr == 22050 and len(audio) == len(texts)
        for b, a in enumerate(audio):
            if a is not None:
                assert done_at[b] is None and a.dtype == np.int16 and a.ndim == 1
                pieces[b].append(a)
            if done[b]:
                assert done_at[b] is None
                done_at[b] = n
        n += 1
    assert n >= 2 and all(v is not None for v in done_at)
    recs = tts.last_stream_latents
    assert len(recs) >= 2 and tts.last_stream.first_chunk_latency is not None
    # lengths: the one-shot synthesis of the same texts (greedy), the tolerance of the v2.5 stream test
    one = tts.infer_batch("spk.wav", texts, None, num_beams=1, top_k=1, max_mel_tokens=30)
    for b in range(len(texts)):
        total = sum(len(p) for p in pieces[b])
        print(f"v2 stream row {b}: {total} samples in {len(pieces[b])} pieces; one-shot {one[b][1].shape[0]}")
        assert abs(total - one[b][1].shape[0]) <= 2 * 256, (b, total, one[b][1].shape)
    # latents: the non-overlapping parts of the chunks, laid end to end, are the one-shot latent pass over the row's final trimmed codes
    codes = torch.cat([r["codes"][:, r["new_from"]:] for r in recs], dim=1).cpu()
    lat = torch.cat([r["latent"][:, r["new_from"]:] for r in recs], dim=1).cpu()
    assert codes.shape[1] == lat.shape[1] and [r["pos"] for r in recs] == [i * (chunk - ovl) for i in range(len(recs))]
    bundle = fe.speaker_bundle("spk.wav")
    spk, emo_feat = bundle["spk_cond_emb"], bundle["emo_cond_emb"]
    lat1 = tts.gpt.get_conditioning(spk.transpose(1, 2), torch.tensor([min(spk.shape[-1], spk.shape[1])], device=spk.device))
    emovec = tts._emovec(dict(tts._speaker("spk.wav")), "spk.wav", 1.0, None, False)
    checked = 0
    for b, t in enumerate(texts):
        seg = fe.text_segments(t, None, 120, True, tts.gpt.n_text_pos)[0]
        ids = seg[:-1].long()[None]                                       # without the Frontend protocol's stop id
        stop = (codes[b] == tts.stop_mel_token).nonzero()
        nb = int(stop[0]) if stop.numel() else codes.shape[1]
        if nb == 0:
            continue
        ref = tts.gpt(lat1, ids.to(DEV), torch.tensor([ids.shape[1]]), codes[b:b + 1, :nb].to(DEV), torch.tensor([nb]), emo_feat,
                      emo_vec=emovec[:1], use_speed=torch.zeros(1, dtype=torch.long)).cpu()
        err = float((lat[b, :nb] - ref[0]).abs().max())
        print(f"v2 stream row {b}: {nb} codes, chunk latents vs the one-shot latent pass on the row alone: max|d| {err:.2e} (bound {ATOL})")
        assert err <= ATOL
        checked += 1
    assert checked >= 2


# ---- 6. argument errors come back as codes with a message ----------------------------------------------------------------------------------
def test_session_argument_errors(golden_dir):
    from indextts_amd import _lib
    z, cfg, sd = _case(golden_dir, "gpt_latent.npz")
    m = _engine(cfg, sd, "fp32")
    L = _lib.lib()
    D, B, P = cfg.model_dim, 2, 12
    x = torch.zeros(B, P, D, device=DEV)
    need = L.itts_gpt_latent_workspace_bytes(m._h, B, P, 6, 4)
    assert need > 0 and L.itts_gpt_latent_workspace_bytes(m._h, 0, P, 6, 4) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = _lib.stream_ptr(DEV)
    s = C.c_void_p()

    def msg():
        return L.itts_last_error().decode()

    lens = (C.c_int32 * B)(12, 13)                                       # a prefix longer than max_prefix
    assert L.itts_gpt_latent_open(m._h, _lib.ptr(x), lens, B, P, 6, 4, _lib.ptr(ws), need, st, C.byref(s)) == _lib.ERR_ARG and "prefix_lens" in msg()
    lens = (C.c_int32 * B)(12, 0)
    assert L.itts_gpt_latent_open(m._h, _lib.ptr(x), lens, B, P, 6, 4, _lib.ptr(ws), need, st, C.byref(s)) == _lib.ERR_ARG
    lens = (C.c_int32 * B)(12, 9)
    assert L.itts_gpt_latent_open(m._h, _lib.ptr(x), lens, B, P, 6, 4, _lib.ptr(ws), 1024, st, C.byref(s)) == _lib.ERR_ARG and "workspace" in msg()
    assert L.itts_gpt_latent_open(m._h, None, lens, B, P, 6, 4, _lib.ptr(ws), need, st, C.byref(s)) == _lib.ERR_ARG
    too_many = int(m._emb["mel_pos_embedding.emb.weight"].shape[0]) + 1
    assert L.itts_gpt_latent_open(m._h, _lib.ptr(x), lens, B, P, too_many, 4, _lib.ptr(ws), need, st, C.byref(s)) == _lib.ERR_ARG and "position table" in msg()
    assert not s.value
    _lib.check(L.itts_gpt_latent_open(m._h, _lib.ptr(x), lens, B, P, 6, 4, _lib.ptr(ws), need, st, C.byref(s)), "itts_gpt_latent_open")
    codes = torch.zeros(B, 5, dtype=torch.int64, device=DEV)
    out = torch.empty(B, 5, D, device=DEV)
    assert L.itts_gpt_latent_append(s, _lib.ptr(codes), 5, _lib.ptr(out), st) == _lib.ERR_ARG and "max_append" in msg()
    assert L.itts_gpt_latent_append(s, _lib.ptr(codes), 0, _lib.ptr(out), st) == _lib.ERR_ARG
    assert L.itts_gpt_latent_append(s, None, 2, _lib.ptr(out), st) == _lib.ERR_ARG
    _lib.check(L.itts_gpt_latent_append(s, _lib.ptr(codes), 4, _lib.ptr(out), st), "itts_gpt_latent_append")
    assert L.itts_gpt_latent_appended(s) == 4
    assert L.itts_gpt_latent_append(s, _lib.ptr(codes), 3, _lib.ptr(out), st) == _lib.ERR_ARG and "max_codes" in msg()
    _lib.check(L.itts_gpt_latent_append(s, _lib.ptr(codes), 2, _lib.ptr(out), st), "itts_gpt_latent_append")
    assert L.itts_gpt_latent_close(s) == 0
    assert L.itts_gpt_latent_append(s, _lib.ptr(codes), 1, _lib.ptr(out), st) == _lib.ERR_STATE and "closed" in msg()
    assert L.itts_gpt_latent_close(s) == _lib.ERR_STATE and L.itts_gpt_latent_appended(s) == -1
    # the host wrapper refuses a closed session too, and an engine with an open session can be dropped
    sess = m.latent_session(torch.zeros(B, 3, D), torch.full((B, 4), 5), torch.tensor([4, 2]), max_codes=4, max_append=4)
    sess.close()
    with pytest.raises(RuntimeError, match="closed"):
        sess.append(torch.zeros(B, 1, dtype=torch.int64))
    keep = m.latent_session(torch.zeros(B, 3, D), torch.full((B, 4), 5), torch.tensor([4, 2]), max_codes=4, max_append=4)
    del m
    keep.close()
