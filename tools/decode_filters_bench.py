"""GPU box: what an installed logits filter costs per decoded token (bf16, sampled, num_beams = 1, hipGraph) -- the shape of decode_bench.py,
the plain call and the filtered call alternated in one process.
usage: decode_filters_bench.py <n_gen> <B,B,...> '<json of generate kwargs>'
e.g.   decode_filters_bench.py 560 64 '{"no_repeat_ngram_size": 4}'"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from indextts_amd import gpt, synth  # noqa: E402

n_gen = int(sys.argv[1]) if len(sys.argv) > 1 else 560
Bs = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "64").split(",")]
filters = json.loads(sys.argv[3]) if len(sys.argv) > 3 else {"no_repeat_ngram_size": 4}
gcfg = dict(synth.GPT_V25)
m = gpt.UnifiedVoice(spk_cond_mode="campplus", **gcfg, precision="bf16", device="cuda:0")
m.load_state_dict(synth.gpt_weights(gcfg, seed=1234, suppress_eos=True))
m.post_init_gpt2_config(kv_cache=True, half=True)
g = torch.Generator().manual_seed(0)
style = torch.randn(1, 192, generator=g).cuda()
emo = (torch.randn(1, 1280, generator=g) * 0.1).cuda()
kw = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.8, num_beams=1, repetition_penalty=10.0, length_penalty=0.0)
for B in Bs:
    text = torch.randint(2, 12000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
    langs = torch.full((B,), 3, dtype=torch.long).cuda()
    best = {}
    for rep in range(4):                                     # round 0 warms both graphs up
        for name, extra in (("plain", {}), ("filtered", filters)):
            m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=n_gen, seed=7, **kw, **extra)
            t = m.last_timing
            ms = t["decode_ms"] / max(1, t["steps"] - 1)
            if rep > 0:
                best[name] = min(ms, best.get(name, ms))
    print(f"B={B:3d} n={n_gen} filters={filters}: plain {best['plain']:.4f} ms/token, filtered {best['filtered']:.4f} ms/token "
          f"(+{(best['filtered'] / best['plain'] - 1) * 100:.2f} %)", flush=True)
