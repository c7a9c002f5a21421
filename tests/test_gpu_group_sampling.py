"""Per-group sampling settings under beam search (`generate(num_beams > 1, group_sampling=, row_max_new=)`, `BeamDecodeSession(group_sampling=)`,
`itts_gpt_set_group_sampling`; design reference: per-request settings in one batch, backends/trt/serving/triton_server.py:96-305, in the
reference's default 3-beam mode, indextts/infer_v2_5.py:732-740).  The contract: group g of a beam batch whose groups carry DIFFERENT settings
(beam search next to beam-sample, own penalties, own length penalty) ends, bit for bit, with the ids group g ends with in the existing scalar
beam call run over the whole batch with group g's settings -- with the seeded device RNG and with a given uniform stream, in the f32 and in
the bf16 engine, with per-group caps, with two beams; a group admitted into a session under its own entry ends with the ids it gets alone;
the num_beams = 1 entries refuse an installed group table.  ("No table = the bits of before" is what the reference-minted beam fixtures of
tests/test_gpu_gpt.py and tests/test_gpu_beam_session.py check.)"""
import os

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1234
MAX_NEW = 40
NB = 3
SETS = [
    dict(do_sample=False, repetition_penalty=1.0, length_penalty=0.0),
    dict(do_sample=False, repetition_penalty=10.0, length_penalty=1.0),
    dict(do_sample=True, temperature=0.8, top_k=30, top_p=0.8, repetition_penalty=10.0, length_penalty=0.0),     # the pipeline's defaults
    dict(do_sample=True, temperature=1.3, top_k=5, top_p=1.0, repetition_penalty=1.0, typical_mass=0.9, length_penalty=1.0),
]
CAPS = [MAX_NEW, 9, 25, 17]


def _engine(cfg, sd, prec):
    from indextts_amd import gpt
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, max_text_tokens=cfg.max_text_tokens,
                         max_mel_tokens=cfg.max_mel_tokens, number_text_tokens=cfg.number_text_tokens, precision=prec, device=DEV)
    m.load_state_dict(sd)
    m.post_init_gpt2_config(kv_cache=True, half=prec == "bf16")
    return m


def _ids(row, stop):
    """the ids of a result row up to its first stop token"""
    row = row.tolist()
    return row[:row.index(stop)] if stop in row else row


def _groups(codes, stop):
    return [_ids(r, stop) for r in codes.cpu()]


def _scalar_kw(s):
    kw = dict(do_sample=s["do_sample"], top_k=s.get("top_k", 50), top_p=s.get("top_p", 1.0), temperature=s.get("temperature", 1.0),
              repetition_penalty=s["repetition_penalty"], length_penalty=s["length_penalty"])
    if s.get("typical_mass"):
        kw.update(typical_sampling=True, typical_mass=s["typical_mass"])
    return kw


_CACHE = {}


def _setup(golden_dir, prec):
    """engine + inputs + the scalar beam references (computed once per precision and shared; nothing below modifies them).  The fixture's EOS
    bias is lowered until every reference group holds >= 8 codes and every group sees >= 3 distinct results over the four scalar runs."""
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
    text = torch.from_numpy(z["text"])[long_row:long_row + 1].repeat(4, 1).contiguous()      # 4 utterances of the longest-running text
    langs = torch.from_numpy(z["langs"])[long_row:long_row + 1].repeat(4).contiguous()
    uniforms = torch.rand(MAX_NEW, 4, 2 * NB, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    picked = None
    for bias in (float(z["eos_bias"]), 0.75 * float(z["eos_bias"]), 0.5 * float(z["eos_bias"]), 0.25 * float(z["eos_bias"]), 0.0):
        sd = G.synth_weights(cfg, seed=int(z["seed"]))
        sd["mel_head.bias"][cfg.stop_mel_token] += bias
        m = _engine(cfg, sd, prec)
        stop = m.stop_mel_token

        def call(n=4, num_beams=NB, **kw):
            return m.inference_speech(None, text[:n].contiguous(), langs=langs[:n].contiguous(), emo_vec=emo, campplus_embedding=style,
                                      max_generate_length=MAX_NEW, num_beams=num_beams, **kw)[0]
        refs = {}
        for name, extra in (("rng", dict(seed=SEED)), ("uniforms", dict(uniforms=uniforms, seed=SEED))):
            refs[name] = [_groups(call(**_scalar_kw(s), **extra), stop) for s in SETS]      # the parent's own path: one scalar beam call per set
        ok = all(len(refs[n][i][i]) >= 8 for n in refs for i in range(4)) and \
            all(len({tuple(refs[n][s][b]) for s in range(4)}) >= 3 for n in refs for b in range(4))
        print(f"{prec}: eos bias {bias}: reference code counts { {n: [len(refs[n][i][i]) for i in range(4)] for n in refs} } -> "
              f"{'ok' if ok else 'rejected'}")
        if ok:
            picked = dict(m=m, call=call, refs=refs, text=text, langs=langs, style=style, emo=emo, uniforms=uniforms, capped=None)
            break
    assert picked is not None, "no EOS bias gives non-trivial scalar beam references"
    _CACHE[prec] = picked
    return picked


def _capped_refs(su):
    """group g of the scalar beam call with set g's settings and the per-group caps CAPS (shared by the cap test and the session test)"""
    if su["capped"] is None:
        stop = su["m"].stop_mel_token
        su["capped"] = [_groups(su["call"](seed=SEED, row_max_new=CAPS, **_scalar_kw(s)), stop)[i] for i, s in enumerate(SETS)]
    return su["capped"]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("stream", ["rng", "uniforms"])
def test_mixed_groups_equal_their_scalar_beam_runs(golden_dir, prec, stream):
    su = _setup(golden_dir, prec)
    m, stop = su["m"], su["m"].stop_mel_token
    table = [dict(s, seed=SEED) for s in SETS]                   # default `stream` (= the slot), every entry's seed = the call's
    extra = dict(seed=SEED) if stream == "rng" else dict(uniforms=su["uniforms"], seed=SEED)
    got = _groups(su["call"](group_sampling=table, do_sample=False, **extra), stop)
    print(f"{prec} {stream}: mixed code counts {[len(g) for g in got]}")
    for i in range(4):
        assert got[i] == su["refs"][stream][i][i], f"group {i} ({SETS[i]}) differs from the scalar beam run with its settings"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_same_entry_in_every_group_is_the_scalar_call(golden_dir, prec):
    su = _setup(golden_dir, prec)
    stop = su["m"].stop_mel_token
    for i in (2, 3):                                             # another call-level seed: the entry's is the one used
        got = _groups(su["call"](group_sampling=[dict(SETS[i], seed=SEED)] * 4, do_sample=False, seed=99), stop)
        for b in range(4):
            assert got[b] == su["refs"]["rng"][i][b], f"set {i} group {b}"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_per_group_caps_on_the_one_shot_path(golden_dir, prec):
    su = _setup(golden_dir, prec)
    stop = su["m"].stop_mel_token
    refs = _capped_refs(su)
    got = _groups(su["call"](group_sampling=[dict(s, seed=SEED) for s in SETS], do_sample=False, seed=SEED, row_max_new=CAPS), stop)
    print(f"{prec}: capped code counts {[len(g) for g in got]} (caps {CAPS})")
    for i in range(4):
        assert len(got[i]) <= CAPS[i]
        assert got[i] == refs[i], f"group {i}"
    # the caps bind: an uncapped reference of a capped group is longer than its cap somewhere
    assert any(len(su["refs"]["rng"][i][i]) > CAPS[i] for i in range(4))


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_two_beams_two_utterances_with_their_own_top_k(golden_dir, prec):
    """num_beams = 2: the smallest shape where the 2 * nb candidates, the union and a per-group ksel all differ from the 3-beam case"""
    su = _setup(golden_dir, prec)
    stop = su["m"].stop_mel_token
    sets = [SETS[2], dict(SETS[2], top_k=5, top_p=1.0)]
    refs = [_groups(su["call"](n=2, num_beams=2, seed=SEED, **_scalar_kw(s)), stop) for s in sets]
    got = _groups(su["call"](n=2, num_beams=2, group_sampling=[dict(s, seed=SEED) for s in sets], do_sample=False, seed=SEED), stop)
    print(f"{prec}: two-beam code counts {[len(g) for g in got]}")
    assert refs[0] != refs[1], "the two settings must lead somewhere else"
    for i in range(2):
        assert len(refs[i][i]) >= 1 and got[i] == refs[i][i], f"group {i}"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_session_admission_under_its_own_entry(golden_dir, prec):
    from indextts_amd import gpt
    su = _setup(golden_dir, prec)
    m, stop, text, langs = su["m"], su["m"].stop_mel_token, su["text"], su["langs"]
    S2 = 4321
    own = SETS[2]
    # the utterance alone: slot 0 of a scalar beam call with seed S2 and its settings
    solo = _groups(su["call"](n=1, seed=S2, **_scalar_kw(own)), stop)[0]
    emb, mask, mn, hf = m.inference_speech_stream(None, text, langs=langs, emo_vec=su["emo"], campplus_embedding=su["style"],
                                                  max_generate_length=MAX_NEW, do_sample=False, seed=SEED)
    caps = [MAX_NEW, 9, MAX_NEW, MAX_NEW]                        # group 1 is free long before the others stop
    with gpt.BeamDecodeSession(m, emb, mask, mn, num_beams=NB, group_sampling=[dict(s, seed=SEED) for s in SETS], row_max_new=caps, **hf) as s:
        s.run(4)
        with pytest.raises(ValueError):
            s.admit([1], emb[:1], mask[:1], row_max_new=[MAX_NEW])    # a session with a table needs the new utterance's entry
        while not s.finished():
            s.run(4)
        slot = s.finished()[0]
        before = s.result(slot).tolist()
        k = s.steps
        assert slot == 1 and k < MAX_NEW - 8, "the admission must happen while the other groups are searching"
        s.admit([slot], emb[:1], mask[:1], row_max_new=[MAX_NEW], group_sampling=[dict(own, stream=0, seed=S2)])
        while len(s.finished()) < 4 and s.steps < 4 * MAX_NEW:
            s.run(4)
        assert len(s.finished()) == 4
        got = [_ids(s.result(b), stop) for b in range(4)]
    print(f"{prec}: admitted at step {k} into slot {slot}: {len(got[slot])} codes, alone {len(solo)}")
    assert len(solo) >= 1
    assert got[slot] == solo, "the admitted utterance must end with the ids it gets alone"
    assert _ids(torch.tensor(before), stop) == _capped_refs(su)[1], "group 1 before the admission: set 1 under its cap of 9"
    for b in (0, 2, 3):
        assert got[b] == su["refs"]["rng"][b][b], f"group {b} was disturbed by the admission"


def test_refusals_and_uninstall_restores_the_scalar_call(golden_dir):
    from indextts_amd import gpt, _lib
    su = _setup(golden_dir, "fp32")
    m, call, stop = su["m"], su["call"], su["m"].stop_mel_token
    before = _groups(call(seed=SEED, **_scalar_kw(SETS[2])), stop)
    defaults = dict(do_sample=0, top_k=50, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_mass=0.0, seed=0, length_penalty=1.0)
    m._install_group_sampling(gpt.group_sampling_entries([dict(s, seed=SEED) for s in SETS], 4, defaults))
    try:
        with pytest.raises(_lib.HipEngineError, match="group sampling table"):          # the group table serves beam calls only
            call(num_beams=1, do_sample=False)
        with pytest.raises(_lib.HipEngineError, match="entries"):                       # a table of 4 does not serve a batch of 1
            call(n=1, do_sample=False)
    finally:
        m._uninstall_group_sampling()
    # a bad entry is rejected by the engine itself (the host check is bypassed here), and nothing is installed
    bad = gpt.group_sampling_entries([dict(SETS[2], seed=SEED)] * 4, 4, defaults)
    bad[1].top_k = 65
    with pytest.raises(_lib.HipEngineError, match="top_k"):
        m._install_group_sampling(bad)
    assert len(_groups(call(num_beams=1, do_sample=False), stop)) == 4                  # nothing installed: num_beams = 1 runs
    after = _groups(call(seed=SEED, **_scalar_kw(SETS[2])), stop)
    for b in range(4):
        assert after[b] == before[b] and before[b] == su["refs"]["rng"][2][b]
