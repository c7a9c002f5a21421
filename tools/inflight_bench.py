#!/usr/bin/env python3
"""GPU box: the GPT stage of N ragged utterances on S decode slots -- in flight (freed slots refilled from the waiting utterances,
UnifiedVoice.inference_speech_inflight) against drained batches of S (row compaction on in both).  Production GPT widths, synthetic weights, EOS
suppressed: every utterance runs to its cap.  usage: inflight_bench.py [N=128] [slots=64] [chunk_tokens=32] [min_free=8] [lo=120] [hi=560]
[--num-beams K]

--num-beams K (K > 1): beam search on S beam GROUPS (UnifiedVoice.inference_speech_inflight_beams) against the same utterances as drained S-group
batches through the unchanged `generate(num_beams=K)` path.  That path takes one max_new_tokens per call, so a drained batch runs to the LONGEST cap
among its utterances -- what draining costs: a group that has finished keeps its rows until the batch ends.  The two are timed alternately in one
process; the idle share of the session's group-steps is printed with the schedule."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from indextts_amd import gpt, synth  # noqa: E402

argv = list(sys.argv[1:])
NB = 1
if "--num-beams" in argv:
    i = argv.index("--num-beams")
    NB = int(argv[i + 1])
    del argv[i:i + 2]
N, S, CHUNK, MINFREE, LO, HI = [int(argv[i]) if len(argv) > i else d for i, d in enumerate((128, 64, 32, 8, 120, 560))]
dev = "cuda:0"
cfg = dict(synth.GPT_V25)
m = gpt.UnifiedVoice(**cfg, spk_cond_mode="campplus", precision="bf16", device=dev)
m.load_state_dict(synth.gpt_weights(cfg, seed=1234, suppress_eos=True))
m.post_init_gpt2_config(kv_cache=True, half=True)
m.set_compaction(True, 8)
g = torch.Generator().manual_seed(308)
caps = torch.randint(LO, HI + 1, (N,), generator=g).tolist()
text = torch.cat([torch.randint(2, 12000, (N, 128), generator=g).to(torch.int32), torch.ones(N, 1, dtype=torch.int32)], dim=1).to(dev)
langs = torch.full((N,), 3, dtype=torch.long, device=dev)
style = (torch.randn(1, 192, generator=g) * 0.1).to(dev)
emo = (torch.randn(1, cfg["model_dim"], generator=g) * 0.1).to(dev)
kw = dict(emo_vec=emo, campplus_embedding=style, max_generate_length=HI, do_sample=True, num_beams=NB, top_p=0.8, top_k=30, temperature=0.8,
          repetition_penalty=10.0)


def drained():
    if NB > 1:
        return [m.inference_speech(None, text[i:i + S], langs=langs[i:i + S], **dict(kw, max_generate_length=max(caps[i:i + S])))[0]
                for i in range(0, N, S)]
    return [m.inference_speech(None, text[i:i + S], langs=langs[i:i + S], row_max_new=caps[i:i + S], **kw)[0] for i in range(0, N, S)]


def inflight():
    if NB > 1:
        k = {a: b for a, b in kw.items() if a != "num_beams"}
        return m.inference_speech_inflight_beams(None, text, langs=langs, slots=S, chunk_tokens=CHUNK, min_free=MINFREE, row_max_new=caps, num_beams=NB,
                                                 **k)[0]
    return m.inference_speech_inflight(None, text, langs=langs, slots=S, chunk_tokens=CHUNK, min_free=MINFREE, row_max_new=caps, **kw)[0]


def wall(fs, rounds=2):
    """best wall time and last result of every function, the functions taking turns (drained, in flight, drained, in flight)"""
    best, res = [None] * len(fs), [None] * len(fs)
    for _ in range(rounds):
        for j, f in enumerate(fs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[j] = f()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best[j] = dt if best[j] is None else min(best[j], dt)
    return best, res


def lens_of(c):
    return [int((r == m.stop_mel_token).nonzero()[0]) if bool((r == m.stop_mel_token).any()) else int(r.numel()) for r in c]


(t_d, t_i), (c_d, c_i) = wall([drained, inflight])
ok = lens_of(c_i) == caps and (NB > 1 or [n for c in c_d for n in lens_of(c)] == caps)      # (a drained beam batch has one budget: its longest cap)
tok = sum(caps)
st = m.last_inflight
if NB > 1:
    # (row_steps charges a whole chunk to every group that was live when the chunk started: a lower bound on the idle share)
    print(f"num_beams={NB}: idle share of the session's group-steps >= {1.0 - st['row_steps'] / max(1, st['slot_steps']):.3f}")
print(f"N={N} slots={S} chunk={CHUNK} min_free={MINFREE} caps {LO}..{HI} (mean {tok / N:.0f}): drained {t_d:.3f} s ({tok / t_d:.0f} tokens/s)  "
      f"in flight {t_i:.3f} s ({tok / t_i:.0f} tokens/s)  speedup {t_d / t_i:.3f}  lengths as capped: {ok}  schedule {m.last_inflight}")
