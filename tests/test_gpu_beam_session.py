"""Beam sessions (`gpt.BeamDecodeSession`, `itts_gpt_generate_beam_chunk`, `itts_gpt_admit_beam_groups`): in-flight batching for the reference's
default generation mode (3-beam beam-sample, infer_v2_5.py:732-740; design reference for the scheduling: backends/trt/serving/triton_server.py:96-305,
backends/trt/pipeline/pipeline.py:459-548).  Engine against engine -- the one-batch beam path is pinned to reference-minted fixtures by
tests/test_gpu_gpt.py::test_beam_codes_bit_exact_vs_reference_golden.  The contract: a session run in chunks is the batch; a group admitted at ANY
session step ends, bit for bit, with the ids it gets in the same slot of a batch decoded from step 0; the groups that were searching are not
disturbed; a group's cap is its max_length; a rejected admission touches nothing."""
import os

import numpy as np
import pytest
import torch

from oracle import gpt_oracle as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_NEW = 40                      # the fixture model's mel position table holds 60 positions
MODES = {"beam": dict(do_sample=False, num_beams=3, repetition_penalty=10.0, length_penalty=0.0),                      # gpt_beam.npz's parameters
         "beam_sample": dict(do_sample=True, num_beams=3, top_p=0.8, top_k=30, temperature=0.8, repetition_penalty=10.0, length_penalty=0.0,
                             seed=20240611),                                                                           # gpt_beam_sample.npz's, seeded
         # beam-sample in which the scorer closes groups early: a length-normalised score and 1.5 more EOS bias than the fixture's
         "beam_sample_closing": dict(do_sample=True, num_beams=3, top_p=0.8, top_k=30, temperature=0.8, repetition_penalty=10.0, length_penalty=1.0,
                                     seed=99)}
EOS_EXTRA = {"beam_sample_closing": 1.5}


def _setup(golden_dir, prec, eos_extra=0.0):
    """The beam fixtures' model (weights, EOS bias) and their five texts: utterances 0-2 open the session, 3 and 4 wait."""
    from indextts_amd import gpt
    z, z2 = np.load(os.path.join(golden_dir, "gpt_beam_sample.npz")), np.load(os.path.join(golden_dir, "gpt_beam.npz"))
    c = z["cfg"]
    cfg = G.GPTConfig(layers=int(c[0]), model_dim=int(c[1]), heads=int(c[2]), max_text_tokens=int(c[3]), max_mel_tokens=int(c[4]),
                      number_text_tokens=int(c[5]))
    sd = G.synth_weights(cfg, seed=int(z["seed"]))
    sd["mel_head.bias"][cfg.stop_mel_token] += float(z["eos_bias"]) + eos_extra
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, max_text_tokens=cfg.max_text_tokens,
                         max_mel_tokens=cfg.max_mel_tokens, number_text_tokens=cfg.number_text_tokens, precision=prec, device=DEV)
    m.load_state_dict(sd)
    m.post_init_gpt2_config(kv_cache=True, half=prec == "bf16")
    text = torch.cat([torch.from_numpy(z["text"]), torch.from_numpy(z2["text"])]).contiguous()
    langs = torch.cat([torch.from_numpy(z["langs"]), torch.from_numpy(z2["langs"])]).contiguous()
    style, emo = torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"])

    def prep(idx, **kw):
        return m.inference_speech_stream(None, text[idx].contiguous(), langs=langs[idx].contiguous(), emo_vec=emo, campplus_embedding=style,
                                         max_generate_length=MAX_NEW, **kw)
    return m, prep, dict(text=text, langs=langs, emo_vec=emo, campplus_embedding=style)


def _ids(row, stop):
    row = row.tolist()
    return row[:row.index(stop)] if stop in row else row


def _to_end(sess, chunk=8, limit=MAX_NEW):
    while len(sess.finished()) < sess.B and sess.steps < limit:
        sess.run(chunk)
    return [sess.result(b).tolist() for b in range(sess.B)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["beam", "beam_sample"])
def test_session_in_chunks_equals_one_batch(golden_dir, prec, mode):
    from indextts_amd import gpt
    m, prep, _ = _setup(golden_dir, prec)
    emb, mask, mn, hf = prep([0, 1, 2], **MODES[mode])
    want = m.generate(emb, mask, mn, **hf).cpu()
    with gpt.BeamDecodeSession(m, emb, mask, mn, **hf) as s:
        got = _to_end(s, chunk=5)
        steps = s.steps
    print(f"{prec} {mode}: session of {steps} steps, lengths {[len(g) for g in got]}")
    for b in range(3):
        assert got[b] == _ids(want[b], m.stop_mel_token), f"group {b}"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["beam", "beam_sample", "beam_sample_closing"])
def test_admitted_group_equals_the_group_from_step_0(golden_dir, prec, mode):
    from indextts_amd import gpt
    m, prep, _ = _setup(golden_dir, prec, EOS_EXTRA.get(mode, 0.0))
    stop = m.stop_mel_token
    kw = MODES[mode]
    emb, mask, mn, hf = prep([0, 1, 2], **kw)
    # beam search: a group of this model is closed by the scorer long before the budget.  Beam-sample with the fixture's parameters
    # (length_penalty 0: sampled candidates keep outscoring the finished hypotheses) closes none before it, so there the slot is freed the other
    # way a group finishes: by its cap; `beam_sample_closing` is the sampled case in which the scorer closes the group.
    capped = mode == "beam_sample"
    hf = dict(hf, row_max_new=[mn, mn, 9] if capped else None)
    # (1) the batch without an admission, polled every 4 steps: the first group to finish frees the slot
    with gpt.BeamDecodeSession(m, emb, mask, mn, **hf) as s0:
        first_fin = None
        while len(s0.finished()) < 3 and s0.steps < mn:
            s0.run(4)
            if first_fin is None and s0.finished():
                first_fin = (s0.finished()[0], s0.steps)
                assert s0.done(first_fin[0]) == (not capped)     # freed by the scorer, or by the cap
        alone = [s0.result(b).tolist() for b in range(3)]
    assert first_fin is not None and first_fin[1] <= mn - 12, f"no group finishes early enough to free a slot: {first_fin}"
    slot = first_fin[0]
    late_slot = [b for b in range(3) if b != slot][0]

    def fresh(at, utt):          # the new utterance in slot `at` of a fresh first batch: the ids every admission into that slot must reproduce
        idx = [0, 1, 2]
        idx[at] = utt
        e, k, n, h = prep(idx, **kw)
        return _ids(m.generate(e, k, n, **h).cpu()[at], stop)
    want_new, want_late = fresh(slot, 3), fresh(late_slot, 4)
    emb3, mask3, _, _ = prep([3], **kw)
    emb4, mask4, _, _ = prep([4], **kw)
    # (2) the same batch; the new utterance takes the freed slot at step k
    with gpt.BeamDecodeSession(m, emb, mask, mn, **hf) as s1:
        while slot not in s1.finished():
            s1.run(4)
        k = s1.steps
        before = s1.result(slot).tolist()
        s1.admit([slot], emb3, mask3)
        assert s1.step0[slot] == k - 1 and slot not in s1.finished()
        with pytest.raises(RuntimeError):        # the caller buffers hold the previous occupant's state until the next run()
            s1.result(slot)
        while len(s1.finished()) < 3 and s1.steps < k + mn:
            s1.run(8)
        admitted = s1.result(slot).tolist()
        others = {b: s1.result(b).tolist() for b in range(3) if b != slot}
        # (3) once more far into the session, past the first batch's budget and the mel position table, into another slot
        while s1.steps < mn + 5 or late_slot not in s1.finished():
            s1.run(8)
        k2 = s1.steps
        s1.admit([late_slot], emb4, mask4)
        while late_slot not in s1.finished() and s1.steps < k2 + mn + 8:
            s1.run(8)
        late = s1.result(late_slot).tolist()
        still = s1.result(slot).tolist()
    print(f"{prec} {mode}: admitted at step {k} into slot {slot} ({len(admitted)} ids) and at step {k2} into slot {late_slot} ({len(late)} ids); "
          f"first batch lengths {[len(a) for a in alone]}")
    assert before == alone[slot]
    for b, v in others.items():
        assert v == alone[b], f"group {b} was disturbed by the admission"
    assert k2 + mn > 60 and k2 > mn
    assert admitted == want_new, "a group admitted into a running session must end with the ids it has in a batch decoded from step 0"
    assert still == want_new, "... and keep them while the session runs on"
    assert late == want_late, "... also when it joins after the session's step counter has passed max_new_tokens"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_inflight_beams_equals_one_batch(golden_dir, prec):
    m, _, args = _setup(golden_dir, prec)
    kw = dict(MODES["beam"], max_generate_length=MAX_NEW, emo_vec=args["emo_vec"], campplus_embedding=args["campplus_embedding"])
    want, _ = m.inference_speech(None, args["text"], langs=args["langs"], **kw)
    for slots in (2, 3):
        got, _ = m.inference_speech_inflight_beams(None, args["text"], langs=args["langs"], slots=slots, chunk_tokens=8, **kw)
        st = m.last_inflight
        print(f"{prec}: in-flight beams on {slots} slots: {st}")
        assert st["sessions"] == 1 and st["admitted"] > 0
        assert torch.equal(got.cpu(), want.cpu()), (slots, got, want)


def test_inflight_beams_at_production_widths_equals_the_utterances_alone():
    """The schedule at the production GPT widths (24 x 1280, bf16): 10 ragged utterances on 3 beam groups, 3-beam search, lengths given as per-utterance
    caps (the synthetic weights never emit the stop token) -- every utterance ends with the ids of `inference_speech(num_beams=3)` on it alone with
    its cap as max_generate_length, all in ONE session whose step counter passes the budget."""
    from indextts_amd import gpt, synth
    cfg = dict(synth.GPT_V25)
    m = gpt.UnifiedVoice(**cfg, spk_cond_mode="campplus", precision="bf16", device=DEV)
    m.load_state_dict(synth.gpt_weights(cfg, seed=1234, suppress_eos=True))
    m.post_init_gpt2_config(kv_cache=True, half=True)
    g = torch.Generator().manual_seed(78)
    n, slots, hi = 10, 3, 20
    caps = torch.randint(5, hi + 1, (n,), generator=g).tolist()
    lens = torch.randint(20, 49, (n,), generator=g).tolist()
    text = torch.ones(n, 48, dtype=torch.int32)
    for i, L in enumerate(lens):
        text[i, :L] = torch.randint(2, 12000, (L,), generator=g).to(torch.int32)
    text = text.to(DEV)
    langs = torch.full((n,), 3, dtype=torch.long, device=DEV)
    style = (torch.randn(1, 192, generator=g) * 0.1).to(DEV)
    emo = (torch.randn(1, cfg["model_dim"], generator=g) * 0.1).to(DEV)
    kw = dict(emo_vec=emo, campplus_embedding=style, do_sample=False, num_beams=3, repetition_penalty=10.0)
    got, _ = m.inference_speech_inflight_beams(None, text, langs=langs, slots=slots, chunk_tokens=8, row_max_new=caps, max_generate_length=hi, **kw)
    st = m.last_inflight
    print(f"production widths: in-flight beam schedule {st}; caps {caps}")
    assert st["sessions"] == 1 and st["admitted"] == n - slots and st["steps"] > hi
    stop = m.stop_mel_token
    for i in range(n):
        ref, _ = m.inference_speech(None, text[i:i + 1], langs=langs[i:i + 1], max_generate_length=caps[i], **kw)
        a, b = _ids(ref[0].cpu(), stop), _ids(got[i].cpu(), stop)
        assert len(a) == caps[i] and a == b, f"utterance {i}: alone {a} vs in flight {b}"


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_group_cap_is_the_groups_max_length(golden_dir, prec):
    from indextts_amd import gpt
    m, prep, _ = _setup(golden_dir, prec)
    emb, mask, mn, hf = prep([0, 1, 2], **MODES["beam"])
    caps = [5, 9, mn]
    with gpt.BeamDecodeSession(m, emb, mask, mn, row_max_new=caps, **hf) as s:
        got = _to_end(s, chunk=8)
    for b, c in enumerate(caps):
        e1, k1, _, h1 = prep([b], **MODES["beam"])
        want = _ids(m.generate(e1, k1, c, **h1).cpu()[0], m.stop_mel_token)
        assert got[b] == want, f"group {b} capped at {c}: {got[b]} vs alone {want}"


def test_rejected_admission_leaves_the_session_alone(golden_dir):
    from indextts_amd import gpt, _lib
    m, prep, _ = _setup(golden_dir, "fp32")
    emb, mask, mn, hf = prep([0, 1, 2], **MODES["beam_sample"])
    emb3, mask3, _, _ = prep([3], **MODES["beam_sample"])
    with gpt.BeamDecodeSession(m, emb, mask, mn, **hf) as s0:
        alone = _to_end(s0)
    with gpt.BeamDecodeSession(m, emb, mask, mn, **hf) as s1:
        s1.run(4)
        busy = [b for b in range(3) if b not in s1.finished()]
        assert busy, "every group had finished after 4 steps"
        with pytest.raises(_lib.HipEngineError):
            s1.admit([busy[0]], emb3, mask3)
        with pytest.raises(_lib.HipEngineError):
            s1.admit([7], emb3, mask3)
        got = _to_end(s1)
    assert got == alone


def test_beam_admission_with_other_parameters_is_a_state_error(golden_dir):
    """`itts_gpt_admit_beam_groups` checks the generation parameters against the suspended loop's (its captured step has them baked in):
    ITTS_ERR_STATE (code 3), and every group ends with the ids of the undisturbed run; the same call with the session's parameters is accepted."""
    import copy
    from indextts_amd import gpt, _lib
    m, prep, _ = _setup(golden_dir, "fp32")
    emb, mask, mn, hf = prep([0, 1, 2], **MODES["beam"])
    emb3, mask3, _, _ = prep([3], **MODES["beam"])
    with gpt.BeamDecodeSession(m, emb, mask, mn, **hf) as s0:
        alone = _to_end(s0)
    with gpt.BeamDecodeSession(m, emb, mask, mn, **hf) as s1:
        while not s1.finished():
            s1.run(4)
        slot = s1.finished()[0]
        before = s1.result(slot).tolist()
        good = s1._gp
        for field, value in (("seed", 12345), ("top_k", 7), ("length_penalty", 1.0)):
            bad = copy.copy(good)
            setattr(bad, field, value)
            s1._gp = bad
            with pytest.raises(_lib.HipEngineError, match="code 3"):
                s1.admit([slot], emb3, mask3)
            s1._gp = good
        assert slot in s1.finished() and s1.result(slot).tolist() == before
        got = _to_end(s1)
        assert got == alone
        s1.admit([slot], emb3, mask3)                # the session's own parameters: accepted
        s1.run(4)
        assert s1.step0[slot] > 0


def test_row_admission_with_other_buffers_or_parameters_is_a_state_error(golden_dir):
    """`itts_gpt_admit_rows` (num_beams = 1) checks `codes_out`, `uniforms` and the generation parameters against the suspended chunk loop's:
    ITTS_ERR_STATE (code 3), the running rows undisturbed."""
    import copy
    from indextts_amd import gpt, _lib
    z = np.load(os.path.join(golden_dir, "gpt_greedy.npz"))
    c = z["cfg"]
    cfg = G.GPTConfig(layers=int(c[0]), model_dim=int(c[1]), heads=int(c[2]), max_text_tokens=int(c[3]), max_mel_tokens=int(c[4]),
                      number_text_tokens=int(c[5]))
    sd = G.synth_weights(cfg, seed=int(z["seed"]))
    sd["mel_head.bias"][cfg.stop_mel_token] += float(z["eos_bias"])
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, max_text_tokens=cfg.max_text_tokens,
                         max_mel_tokens=cfg.max_mel_tokens, number_text_tokens=cfg.number_text_tokens, precision="fp32", device=DEV)
    m.load_state_dict(sd)
    m.post_init_gpt2_config(kv_cache=True, half=False)
    g = z["gen"]
    kw = dict(do_sample=bool(g[0]), num_beams=1, top_p=float(g[2]), top_k=int(g[3]), temperature=float(g[4]), repetition_penalty=float(g[5]))
    text, langs = torch.from_numpy(z["text"]), torch.from_numpy(z["langs"])
    style, emo = torch.from_numpy(z["style"]), torch.from_numpy(z["emo_vec"])
    max_new = min(96, cfg.max_mel_tokens - 2)
    emb, mask, mn, hf = m.inference_speech_stream(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=max_new, **kw)
    B = text.shape[0]

    def to_end(s):
        while s.steps < max_new and len(s.finished()) < B:
            s.run(8)
        return [s.codes(b).tolist() for b in range(B)]
    with gpt.DecodeSession(m, emb, mask, mn, **hf) as s0:
        alone = to_end(s0)
    with gpt.DecodeSession(m, emb, mask, mn, **hf) as s1:
        while not s1.finished():
            s1.run(8)
        slot = s1.finished()[0]
        good_gp, good_codes = s1._gp, s1._codes
        s1._codes = torch.empty_like(good_codes)                  # another code buffer than the loop's captured step writes
        with pytest.raises(_lib.HipEngineError, match="code 3"):
            s1.admit([slot], emb[slot:slot + 1], mask[slot:slot + 1])
        s1._codes = good_codes
        bad = copy.copy(good_gp)
        bad.seed = 4711
        s1._gp = bad
        with pytest.raises(_lib.HipEngineError, match="code 3"):
            s1.admit([slot], emb[slot:slot + 1], mask[slot:slot + 1])
        s1._gp = good_gp
        assert to_end(s1) == alone
