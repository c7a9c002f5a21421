"""Per-slot sampling settings in one decode batch (`generate(..., row_sampling=)`, `itts_gpt_set_row_sampling`; design reference: per-request
settings in one batch, backends/trt/serving/triton_server.py:96-305).  The contract: row i of a batch whose rows carry DIFFERENT sampling
settings generates, bit for bit, the ids row i generates in the existing scalar call run over the whole batch with row i's settings -- with
and without row compaction, with the seeded device RNG and with a given uniform stream, in the f32 and in the bf16 engine; an utterance
admitted into a session under its own entry generates the ids it generates alone; beam calls refuse an installed table."""
import os

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1234
MAX_NEW = 40
SETS = [
    dict(do_sample=False, repetition_penalty=1.0),
    dict(do_sample=False, repetition_penalty=10.0),
    dict(do_sample=True, temperature=0.8, top_k=30, top_p=0.8, repetition_penalty=10.0),
    dict(do_sample=True, temperature=1.3, top_k=5, top_p=1.0, repetition_penalty=1.0, typical_mass=0.9),
]


def _engine(cfg, sd, prec):
    from indextts_amd import gpt
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, max_text_tokens=cfg.max_text_tokens,
                         max_mel_tokens=cfg.max_mel_tokens, number_text_tokens=cfg.number_text_tokens, precision=prec, device=DEV)
    m.load_state_dict(sd)
    m.post_init_gpt2_config(kv_cache=True, half=prec == "bf16")
    return m


def _rows(codes, stop):
    """every row up to and including its first stop token"""
    out = []
    for r in codes.cpu():
        hit = (r == stop).nonzero()
        out.append(r[: int(hit[0]) + 1].clone() if hit.numel() else r.clone())
    return out


def _n_codes(row, stop):
    return int(row.numel()) - int(row.numel() > 0 and int(row[-1]) == stop)


_CACHE = {}


def _setup(golden_dir, prec):
    """engine + inputs + the scalar references (computed once per precision and shared; nothing below modifies them).  The fixture's EOS bias
    is lowered until every reference row holds >= 8 codes and every row sees >= 3 distinct sequences over the four scalar runs."""
    if prec in _CACHE:
        return _CACHE[prec]
    z = np.load(os.path.join(golden_dir, "gpt_greedy.npz"))
    c = z["cfg"]
    cfg = G.GPTConfig(layers=int(c[0]), model_dim=int(c[1]), heads=int(c[2]), max_text_tokens=int(c[3]), max_mel_tokens=int(c[4]),
                      number_text_tokens=int(c[5]))
    style, emo = torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"])
    ref_codes = z["codes"]
    stop_id = int(ref_codes.max())
    ref_lens = [int((r == stop_id).argmax()) if (r == stop_id).any() else r.shape[0] for r in ref_codes]
    long_row = int(np.argmax(ref_lens))
    text = torch.from_numpy(z["text"])[long_row:long_row + 1].repeat(4, 1).contiguous()      # 4 rows of the longest-running text
    langs = torch.from_numpy(z["langs"])[long_row:long_row + 1].repeat(4).contiguous()
    uniforms = torch.rand(MAX_NEW, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    picked = None
    for bias in (float(z["eos_bias"]), 0.75 * float(z["eos_bias"]), 0.5 * float(z["eos_bias"]), 0.25 * float(z["eos_bias"]), 0.0):
        sd = G.synth_weights(cfg, seed=int(z["seed"]))
        sd["mel_head.bias"][cfg.stop_mel_token] += bias
        m = _engine(cfg, sd, prec)
        stop = m.stop_mel_token

        def call(**kw):
            return m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=1,
                                      **kw)[0]
        refs = {}
        for name, extra in (("rng", dict(seed=SEED)), ("uniforms", dict(uniforms=uniforms, seed=SEED))):
            runs = [_rows(call(**_scalar_kw(s), **extra), stop) for s in SETS]          # the parent's own path: one scalar call per set
            refs[name] = runs
        ok = all(_n_codes(refs[n][i][i], stop) >= 8 for n in refs for i in range(4)) and \
            all(len({tuple(refs[n][s][b].tolist()) for s in range(4)}) >= 3 for n in refs for b in range(4))
        print(f"{prec}: eos bias {bias}: reference code counts "
              f"{ {n: [_n_codes(refs[n][i][i], stop) for i in range(4)] for n in refs} } -> {'ok' if ok else 'rejected'}")
        if ok:
            picked = (m, call, refs, text, langs, style, emo, uniforms)
            break
    assert picked is not None, "no EOS bias gives non-trivial scalar references"
    _CACHE[prec] = picked
    return picked


def _scalar_kw(s):
    kw = dict(do_sample=s["do_sample"], top_k=s.get("top_k", 50), top_p=s.get("top_p", 1.0), temperature=s.get("temperature", 1.0),
              repetition_penalty=s["repetition_penalty"])
    if s.get("typical_mass"):
        kw.update(typical_sampling=True, typical_mass=s["typical_mass"])
    return kw


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("compaction", [True, False])
@pytest.mark.parametrize("stream", ["rng", "uniforms"])
def test_mixed_rows_equal_their_scalar_runs(golden_dir, prec, compaction, stream):
    m, call, refs, *_, uniforms = _setup(golden_dir, prec)
    stop = m.stop_mel_token
    table = [dict(s, seed=SEED) for s in SETS]                   # default `stream` (= the slot), every entry's seed = the call's
    m.set_compaction(compaction, 1)                              # buckets of one row: a batch of 4 does compact
    try:
        extra = dict(seed=SEED) if stream == "rng" else dict(uniforms=uniforms, seed=SEED)
        got = _rows(call(row_sampling=table, do_sample=False, **extra), stop)
        stats = dict(m.last_timing)
    finally:
        m.set_compaction(True, 8)
    print(f"{prec} compaction={compaction} {stream}: mixed code counts {[_n_codes(r, stop) for r in got]}, compactions {stats['compactions']}, "
          f"row_steps {stats['row_steps']} of {stats['steps']} steps")
    for i in range(4):
        assert torch.equal(got[i], refs[stream][i][i]), f"row {i} ({SETS[i]}) differs from the scalar run with its settings"
    if not compaction:
        assert stats["compactions"] == 0


CAPS = [MAX_NEW, 9, 25, 17]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_mixed_rows_leaving_a_compacted_batch_at_ragged_steps(golden_dir, prec):
    """the same contract with per-row token caps (`row_max_new`, as merged requests carry them): rows leave the running batch at different
    steps, so the compacted step really reads entry `row_slot[b]`, not entry b"""
    m, call, *_ = _setup(golden_dir, prec)
    stop = m.stop_mel_token
    m.set_compaction(True, 1)
    try:
        refs = [_rows(call(seed=SEED, row_max_new=CAPS, **_scalar_kw(s)), stop)[i] for i, s in enumerate(SETS)]
        got = _rows(call(row_sampling=[dict(s, seed=SEED) for s in SETS], do_sample=False, seed=SEED, row_max_new=CAPS), stop)
        stats = dict(m.last_timing)
    finally:
        m.set_compaction(True, 8)
    print(f"{prec}: capped code counts {[_n_codes(r, stop) for r in got]}, compactions {stats['compactions']}, row_steps {stats['row_steps']}")
    assert [_n_codes(r, stop) for r in refs] == [min(c, _n_codes(r, stop)) for c, r in zip(CAPS, refs)] and stats["compactions"] >= 1
    for i in range(4):
        assert torch.equal(got[i], refs[i]), f"row {i}"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_same_entry_in_every_row_is_the_scalar_call(golden_dir, prec):
    m, call, refs, *_ = _setup(golden_dir, prec)
    stop = m.stop_mel_token
    for i in (2, 3):
        got = _rows(call(row_sampling=[dict(SETS[i], seed=SEED)] * 4, do_sample=False, seed=99), stop)
        for b in range(4):
            assert torch.equal(got[b], refs["rng"][i][b]), f"set {i} row {b}"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_admission_under_its_own_entry(golden_dir, prec):
    from indextts_amd import gpt
    m, call, refs, text, langs, style, emo, _ = _setup(golden_dir, prec)
    stop = m.stop_mel_token
    S2 = 4321
    own = SETS[2]
    # the utterance alone: slot 0 of a scalar call with seed S2 and its settings
    solo = _rows(m.inference_speech(None, text[:1], langs=langs[:1], emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW,
                                    num_beams=1, seed=S2, **_scalar_kw(own))[0], stop)[0]
    emb, mask, mn, hf = m.inference_speech_stream(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW,
                                                  do_sample=False, num_beams=1, seed=SEED)
    hf.pop("uniforms", None)
    emb_n, mask_n = emb[:1], mask[:1]
    caps = [MAX_NEW, 9, MAX_NEW, MAX_NEW]                        # slot 1 is free long before the others stop
    with gpt.DecodeSession(m, emb, mask, mn, row_sampling=[dict(s, seed=SEED) for s in SETS], row_max_new=caps, **hf) as s:
        s.run(8)
        with pytest.raises(ValueError):
            s.admit([0], emb_n, mask_n, row_max_new=[MAX_NEW])   # a session with a table needs the new utterance's entry
        while not s.finished():
            s.run(8)
        slot = s.finished()[0]
        before = s.codes(slot).cpu()
        k = s.steps
        assert slot == 1 and k < MAX_NEW - 8, "the admission must happen while the other rows are running"
        s.admit([slot], emb_n, mask_n, row_max_new=[MAX_NEW], row_sampling=[dict(own, stream=0, seed=S2)])
        while len(s.finished()) < 4 and s.steps < 4 * MAX_NEW:
            s.run(8)
        admitted = s.codes(slot).cpu()
        others = {b: s.codes(b).cpu() for b in range(4) if b != slot}
    print(f"{prec}: admitted at step {k} into slot {slot}: {admitted.numel()} codes, alone {_n_codes(solo, stop)}")
    assert _n_codes(solo, stop) >= 1
    assert torch.equal(admitted, solo[: _n_codes(solo, stop)]), "the admitted utterance must generate the ids it generates alone"
    assert torch.equal(before, refs["rng"][slot][slot][: caps[slot]])
    for b, v in others.items():
        assert torch.equal(v, refs["rng"][b][b][: _n_codes(refs["rng"][b][b], stop)]), f"row {b} was disturbed by the admission"


def test_beams_refuse_a_table_and_uninstall_restores_the_scalar_call(golden_dir):
    from indextts_amd import gpt, _lib
    m, call, refs, text, langs, style, emo, _ = _setup(golden_dir, "fp32")
    stop = m.stop_mel_token
    before = _rows(call(seed=SEED, **_scalar_kw(SETS[2])), stop)
    with pytest.raises(NotImplementedError):
        m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=3,
                           do_sample=False, row_sampling=[dict(SETS[0])] * 4)
    entries = gpt.row_sampling_entries([dict(s, seed=SEED) for s in SETS], 4, dict(do_sample=0, top_k=50, top_p=1.0, temperature=1.0,
                                                                                     repetition_penalty=1.0, typical_mass=0.0, seed=0))
    m._install_row_sampling(entries)
    try:
        with pytest.raises(_lib.HipEngineError, match="sampling table"):
            m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=3,
                               do_sample=False)
        with pytest.raises(_lib.HipEngineError, match="entries"):                      # a table of 4 does not serve a batch of 1
            m.inference_speech(None, text[:1], langs=langs[:1], emo_vec=emo, campplus_embedding=style, max_generate_length=MAX_NEW, num_beams=1,
                               do_sample=False)
    finally:
        m._uninstall_row_sampling()
    # a bad entry is rejected by the engine itself (the host check is bypassed here), and nothing is installed
    bad = gpt.row_sampling_entries([dict(SETS[2], seed=SEED)] * 4, 4, dict(do_sample=0, top_k=50, top_p=1.0, temperature=1.0,
                                                                          repetition_penalty=1.0, typical_mass=0.0, seed=0))
    bad[1].top_k = 65
    with pytest.raises(_lib.HipEngineError, match="top_k"):
        m._install_row_sampling(bad)
    after = _rows(call(seed=SEED, **_scalar_kw(SETS[2])), stop)
    for b in range(4):
        assert torch.equal(after[b], before[b]) and torch.equal(before[b], refs["rng"][2][b])
