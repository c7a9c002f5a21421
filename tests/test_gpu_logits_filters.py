"""Device logits filters (`itts_gpt_set_logits_filters`): the generate() kwargs min_new_tokens, min_length, no_repeat_ngram_size, suppress_tokens,
begin_suppress_tokens, single-token bad_words_ids, exponential_decay_length_penalty, min_p, epsilon_cutoff and eta_cutoff inside the selection
kernels.  The f32 engine is held, id for id, to what the REFERENCE's own generate() produced with the same kwargs (tests/golden/gpt_filters_*.npz,
tools/make_golden_gpt_filters.py); sessions, chunks and the bf16 engine are held to properties and to the engine decoding the same row alone."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = ("minnew", "minnew4", "minlen", "ngram2", "ngram3", "suppress", "decay", "sample_minp", "sample_epsilon", "sample_eta", "sample_order",
        "beam_sample", "beam_suppress")


def _cfg(c):
    return G.GPTConfig(layers=int(c[0]), model_dim=int(c[1]), heads=int(c[2]), max_text_tokens=int(c[3]), max_mel_tokens=int(c[4]),
                       number_text_tokens=int(c[5]))


def _engine(cfg, sd, prec="fp32"):
    from indextts_amd import gpt
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, max_text_tokens=cfg.max_text_tokens,
                         max_mel_tokens=cfg.max_mel_tokens, number_text_tokens=cfg.number_text_tokens, precision=prec, device=DEV)
    m.load_state_dict(sd)
    m.post_init_gpt2_config(kv_cache=True, half=prec == "bf16")
    return m


def _load(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, f"gpt_filters_{tag}.npz"))
    cfg = _cfg(z["cfg"])
    sd = G.synth_weights(cfg, seed=int(z["seed"]))
    sd["mel_head.bias"][cfg.stop_mel_token] += float(z["eos_bias"])
    sd["mel_head.bias"][1] += float(z["one_bias"])
    return z, cfg, sd


def _base_kw(z):
    g = z["gen"]
    return dict(do_sample=bool(g[0]), num_beams=int(g[1]), top_p=float(g[2]), top_k=int(g[3]), temperature=float(g[4]),
                repetition_penalty=float(g[5]), length_penalty=float(g[6]))


def _filter_kw(z):
    kw = json.loads(str(z["kwargs"]))
    if "exponential_decay_length_penalty" in kw:
        kw["exponential_decay_length_penalty"] = tuple(kw["exponential_decay_length_penalty"])
    return kw


def _run(m, z, **filters):
    kw = _base_kw(z)
    u = torch.from_numpy(z["uniforms"])
    if kw["num_beams"] == 1:
        u = u[..., 0]
    codes, _ = m.inference_speech(None, torch.from_numpy(z["text"]), langs=torch.from_numpy(z["langs"]), emo_vec=torch.from_numpy(z["emo_vec"]),
                                  campplus_embedding=torch.from_numpy(z["style"]), max_generate_length=int(z["max_gen"]),
                                  uniforms=u if kw["do_sample"] else None, **kw, **filters)
    return codes.cpu().numpy()


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)[0]
        pytest.fail(f"{what}: first divergence at (row, step) = {bad.tolist()}: got {got[tuple(bad)]} want {want[tuple(bad)]}")


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("use_graph", [True, False])
def test_ids_equal_the_references_generate(golden_dir, tag, use_graph):
    """f32 engine: the ids of the reference's own generate() with the same kwargs -- which are NOT the ids of the plain call"""
    z, cfg, sd = _load(golden_dir, tag)
    m = _engine(cfg, sd)
    m.use_graph = use_graph
    got = _run(m, z, **_filter_kw(z))
    print(f"{tag} graph={use_graph}: kwargs {_filter_kw(z)}, ids {got.shape}, the plain run's {z['codes_plain'].shape}")
    _same(got, z["codes"], tag)


def test_one_graph_serves_every_installation_and_nothing_sticks(golden_dir):
    """One engine handle, the same shapes, the graph on: a filtered call, a plain call, the filtered call with another min_new_tokens, the first
    call again -- each with its own fixture's ids (a step graph that baked a setting in, or a filter left installed, would repeat another
    call's), the two later filtered calls replayed from the first one's captured step."""
    za, cfg, sd = _load(golden_dir, "minnew")
    zb, _, _ = _load(golden_dir, "minnew4")
    plain = np.load(os.path.join(golden_dir, "gpt_greedy.npz"))["codes"]
    m = _engine(cfg, sd)
    m.use_graph = True
    _same(_run(m, za, **_filter_kw(za)), za["codes"], "filtered call")
    _same(_run(m, za), plain, "plain call after a filtered one")
    cap = m.graph_stats()
    _same(_run(m, zb, **_filter_kw(zb)), zb["codes"], "filtered call, another min_new_tokens")
    _same(_run(m, za, **_filter_kw(za)), za["codes"], "the first filtered call again")
    now = m.graph_stats()
    print(f"graphs captured {cap['captures']} -> {now['captures']}, reused {cap['hits']} -> {now['hits']}")
    assert now["captures"] == cap["captures"] and now["hits"] >= cap["hits"] + 2       # the settings live in device memory, not in the graph
    _same(_run(m, za), plain, "plain call at the end")


def _ngram_model(eos_bias):
    """the n = 3 fixture's model (a bias towards id 1 makes the n-gram filter bite every third token) with a stop bias of the test's own"""
    cfg = G.GPTConfig(max_text_tokens=40, max_mel_tokens=60, number_text_tokens=200, layers=2, model_dim=128, heads=2)
    sd = G.synth_weights(cfg, seed=52)
    sd["mel_head.bias"][cfg.stop_mel_token] += eos_bias
    sd["mel_head.bias"][1] += 6.0
    return cfg, sd


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_admitted_row_counts_from_its_own_first_token(prec):
    """DecodeSession with min_new_tokens = K and n-gram 3: a row admitted at a session step > K -- with a shorter prompt than the session's --
    generates bit for bit what it generates alone (its own step, its own code history, its own prompt length)."""
    from indextts_amd import gpt
    K = 8
    cfg, sd = _ngram_model(4.0)
    m = _engine(cfg, sd, prec)
    g = torch.Generator().manual_seed(152)
    text = torch.randint(2, cfg.number_text_tokens, (3, 9), generator=g)
    text[1, 6:] = 1
    text[2, 8:] = 1
    style, emo = torch.randn(1, 192, generator=g), torch.randn(1, cfg.model_dim, generator=g) * 0.1
    langs = torch.randint(0, cfg.n_langs, (3,), generator=g)
    kw = dict(do_sample=False, num_beams=1, repetition_penalty=1.0, no_repeat_ngram_size=3, min_new_tokens=K)
    prep = lambda t, lg: m.inference_speech_stream(None, t, langs=lg, emo_vec=emo, campplus_embedding=style, max_generate_length=40, **kw)
    emb, mask, mn, hf = prep(text, langs)
    emb_n, mask_n, _, _ = prep(text[1:2, :6].contiguous(), langs[1:2])
    assert emb_n.shape[1] < emb.shape[1]
    stop = m.stop_mel_token
    solo = m.generate(emb_n, mask_n, mn, **hf).cpu()[0].tolist()
    solo = solo[:solo.index(stop)] if stop in solo else solo
    plain_kw = {k: v for k, v in hf.items() if k not in ("no_repeat_ngram_size", "min_new_tokens")}
    unfiltered = m.generate(emb_n, mask_n, mn, **plain_kw).cpu()[0].tolist()
    assert len(solo) >= K and solo != unfiltered[:len(solo)]                      # the filters bite on this row
    with gpt.DecodeSession(m, emb, mask, mn, **hf) as s:
        while not s.finished() and s.steps < mn:
            s.run(8)
        k, slot = s.steps, s.finished()[0]
        assert k > K
        s.admit([slot], emb_n, mask_n)
        while slot not in s.finished() and s.steps < k + mn:
            s.run(8)
        admitted = s.codes(slot).cpu().tolist()
    print(f"{prec}: admitted at session step {k} into slot {slot}: {admitted}; alone {solo}; without filters {unfiltered[:12]}")
    assert admitted == solo
    assert m.generate(emb_n, mask_n, mn, **plain_kw).cpu()[0].tolist() == unfiltered    # close() cleared the session's filters


def test_admitted_beam_group_counts_from_its_own_first_step(golden_dir):
    """BeamDecodeSession with min_new_tokens = K: a group admitted at a session step > K ends with the ids it gets alone"""
    from indextts_amd import gpt
    K = 7
    z, z2 = np.load(os.path.join(golden_dir, "gpt_beam_sample.npz")), np.load(os.path.join(golden_dir, "gpt_beam.npz"))
    cfg = _cfg(z["cfg"])
    sd = G.synth_weights(cfg, seed=int(z["seed"]))
    sd["mel_head.bias"][cfg.stop_mel_token] += float(z["eos_bias"]) + 1.5
    m = _engine(cfg, sd)
    style, emo = torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"])
    kw = dict(do_sample=False, num_beams=3, repetition_penalty=10.0, length_penalty=1.0, min_new_tokens=K)
    prep = lambda t, lg: m.inference_speech_stream(None, t, langs=lg, emo_vec=emo, campplus_embedding=style, max_generate_length=40, **kw)
    emb, mask, mn, hf = prep(torch.from_numpy(z["text"]), torch.from_numpy(z["langs"]))
    emb_n, mask_n, _, _ = prep(torch.from_numpy(z2["text"])[1:2, :6].contiguous(), torch.from_numpy(z2["langs"])[1:2])
    stop = m.stop_mel_token
    ids = lambda row: row[:row.index(stop)] if stop in row else row
    alone = ids(m.generate(emb_n, mask_n, mn, **hf).cpu()[0].tolist())
    plain = ids(m.generate(emb_n, mask_n, mn, **{k: v for k, v in hf.items() if k != "min_new_tokens"}).cpu()[0].tolist())
    with gpt.BeamDecodeSession(m, emb, mask, mn, **hf) as s:
        while not s.finished() and s.steps < mn:
            s.run(4)
        k, slot = s.steps, s.finished()[0]
        assert k > K
        s.admit([slot], emb_n, mask_n)
        while slot not in s.finished() and s.steps < k + mn:
            s.run(4)
        admitted = s.result(slot).tolist()
    print(f"admitted at session step {k} into slot {slot}: {len(admitted)} ids, alone {len(alone)}, without min_new_tokens {len(plain)}")
    assert len(plain) < K <= len(alone)                       # the filter bites on this utterance
    assert admitted == alone


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_properties_hold_in_every_row(prec):
    """8 rows, seeded sampling: no stop token before min_new_tokens, no repeated n-gram over the virtual sequence [1] * (S - 1) + [start_mel] +
    codes, no suppressed id anywhere, no begin-suppressed id at position 0 -- whatever the precision."""
    K, n = 10, 3
    cfg, sd = _ngram_model(4.0)
    m = _engine(cfg, sd, prec)
    g = torch.Generator().manual_seed(7)
    lens = [9, 4, 7, 9, 5, 8, 6, 3]
    text = torch.randint(2, cfg.number_text_tokens, (8, 9), generator=g)
    for b, ln in enumerate(lens):
        text[b, ln:] = 1
    style, emo = torch.randn(1, 192, generator=g), torch.randn(1, cfg.model_dim, generator=g) * 0.1
    langs = torch.randint(0, cfg.n_langs, (8,), generator=g)
    base = dict(do_sample=True, num_beams=1, top_p=1.0, top_k=30, temperature=1.0, repetition_penalty=1.0, seed=11)
    call = lambda **kw: m.inference_speech_stream(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=40, **base, **kw)
    emb, mask, mn, hf = call()
    free = m.generate(emb, mask, mn, **hf).cpu().numpy()
    seen = free[(free > 1) & (free != m.stop_mel_token)].ravel()
    common = sorted(set([int(v) for v in np.bincount(seen).argsort()[::-1][:3]] if seen.size else []) | {6546, 1769})   # (and two ids greedy decoding favours)
    begin = [int(v) for v in set(free[:, 0].tolist())]
    emb, mask, mn, hf = call(min_new_tokens=K, no_repeat_ngram_size=n, suppress_tokens=common, begin_suppress_tokens=begin)
    codes = m.generate(emb, mask, mn, **hf).cpu().numpy()
    S, stop = emb.shape[1] + 1, m.stop_mel_token
    print(f"{prec}: suppress {common}, begin-suppress {begin}; unfiltered lengths "
          f"{[int((r == stop).argmax()) if (r == stop).any() else len(r) for r in free]}")
    assert 1 in begin                                         # (the model's favourite first id: the begin filter bites)
    for b, row in enumerate(codes.tolist()):
        end = row.index(stop) if stop in row else len(row)
        own = row[:end + 1]                                   # up to and including the stop token: it was chosen under the filters as well
        assert end >= K, f"row {b} stops at {end} < {K}"
        assert not set(own) & set(common), f"row {b} holds a suppressed id: {own}"
        assert own[0] not in begin, f"row {b} starts with a begin-suppressed id: {own[:3]}"
        seq = [1] * (S - 1) + [m.start_mel_token] + own
        grams = [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
        rep = [t for i, t in enumerate(grams) if i + n > S and t in grams[:i]]       # n-grams that end in a generated id
        assert not rep, f"row {b} repeats the {n}-gram {rep[0]}: {own}"
        print(f"  row {b}: {end} codes, {own[:10]}")


def test_chunks_are_the_chunks_of_the_one_shot_call(golden_dir):
    """generate_chunks with filters yields the one-shot filtered call's codes, chunk by chunk, and leaves nothing installed"""
    z, cfg, sd = _load(golden_dir, "minnew")
    m = _engine(cfg, sd)
    kw = dict(_base_kw(z), **_filter_kw(z))
    emb, mask, mn, hf = m.inference_speech_stream(None, torch.from_numpy(z["text"]), langs=torch.from_numpy(z["langs"]),
                                                  emo_vec=torch.from_numpy(z["emo_vec"]), campplus_embedding=torch.from_numpy(z["style"]),
                                                  max_generate_length=int(z["max_gen"]), **kw)
    want = m.generate(emb, mask, mn, **hf).cpu()
    _same(want.numpy(), z["codes"], "one-shot call")
    full = torch.full((want.shape[0], mn), m.stop_mel_token, dtype=torch.int64)
    full[:, :want.shape[1]] = want
    chunk, overlap = 8, 2
    n = 0
    for i, (c, last, done, lens) in enumerate(m.generate_chunks(emb, mask, mn, chunk, overlap, **hf)):
        pos = i * (chunk - overlap)
        assert torch.equal(c.cpu(), full[:, pos:pos + c.shape[1]]), (i, c.cpu(), full[:, pos:pos + c.shape[1]])
        n += 1
    assert n >= 2 and last
    plain = np.load(os.path.join(golden_dir, "gpt_greedy.npz"))["codes"]
    _same(_run(m, z), plain, "plain call after the stream")
