"""GPU box: streamed IndexTTS-2, the GPT side of a stream -- what the latents of every chunk cost.
Production widths (24 x 1280 x 20 heads, 34 conditioning tokens, 128 text tokens, bf16 engine, sampled, num_beams = 1, hipGraph), a budget of
`max_codes` codes (EOS suppressed: every row runs the whole budget), chunks of `chunk` codes overlapping by `overlap`.  Per batch size:
  * time to the first chunk: prefill + `chunk` decode steps + the first chunk's latents, i.e. until (codes, latents) of chunk 0 can go to
    codes -> mel -> waveform (that stage is NOT part of this tool: bench.py times it);
  * per chunk, the latent cost of (a) the KV-cached session (`UnifiedVoice.latent_session`: append the chunk's new codes) and of (b) the
    one-shot pass over all codes so far (`forward_latent`, all there was before the session; it cannot run beside the suspended decode loop,
    so it is timed after the stream on the same code prefixes).
Every time is a host clock around work that ends in a device synchronisation; the stream runs twice per batch size, the second run is reported.
usage: stream_v2_bench.py [B,B,...] [max_codes] [chunk] [overlap] [out_dir]      (defaults: 1,16  1500  100  20  profiles/stream_v2)"""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from indextts_amd import gpt, synth  # noqa: E402

Bs = [int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "1,16").split(",")]
max_codes = int(sys.argv[2]) if len(sys.argv) > 2 else 1500
chunk = int(sys.argv[3]) if len(sys.argv) > 3 else 100
overlap = int(sys.argv[4]) if len(sys.argv) > 4 else 20
out_dir = sys.argv[5] if len(sys.argv) > 5 else os.path.join("profiles", "stream_v2")
assert torch.cuda.is_available(), "stream_v2_bench.py measures on the GPU: no device, no number"
DEV = "cuda:0"

gcfg = {k: synth.GPT_V25[k] for k in ("layers", "model_dim", "heads", "max_text_tokens", "max_mel_tokens", "number_text_tokens")}
D = gcfg["model_dim"]
g = torch.Generator().manual_seed(0)
sd = dict(synth.gpt_weights(dict(synth.GPT_V25), seed=1234, suppress_eos=True))
sd["speed_emb.weight"] = torch.randn(2, D, generator=g) * 0.3
spk = (torch.randn(1, 32, D, generator=g) * 0.3).to(DEV)
emo = (torch.randn(1, D, generator=g) * 0.1).to(DEV)
m = gpt.UnifiedVoice(**gcfg, precision="bf16", device=DEV, conditioning_fn=lambda x, lengths=None: spk)
m.load_state_dict(sd)
m.post_init_gpt2_config(kv_cache=True, half=True)
kw = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.8, num_beams=1, repetition_penalty=10.0, length_penalty=0.0, seed=7)


def sync():
    torch.cuda.synchronize()


def stream(B):
    text = torch.randint(2, 12000, (B, 128), generator=torch.Generator().manual_seed(B)).to(DEV)
    tl = torch.full((B,), 128)
    conds = m.conds_latent_v2(spk.expand(B, -1, -1), emo)
    emb, mask, max_new, hf = m.inference_speech_stream(None, text, chunk, overlap, emo_vec=emo, conds_latent=conds, max_generate_length=max_codes, **kw)
    lconds = m.latent_conds(spk.expand(B, -1, -1), emo.expand(B, -1), torch.zeros(B, dtype=torch.long))
    sync()
    t0 = time.perf_counter()
    sess = m.latent_session(lconds, text, tl, max_codes=max_new, max_append=chunk)
    sync()
    t_open = time.perf_counter() - t0
    rows, appended, k, first, all_codes = [], 0, 0, None, []
    t_prev = time.perf_counter()
    for codes, is_last, done, lens in m.generate_chunks(emb, mask, max_new, chunk, overlap, **hf):
        sync()
        t_dec = time.perf_counter() - t_prev                 # decode steps since the previous chunk (the first: prefill + `chunk` steps)
        pos = k * (chunk - overlap)
        new = codes[:, appended - pos:]
        t1 = time.perf_counter()
        if new.shape[1]:
            sess.append(new)
            all_codes.append(new)
        sync()
        t_a = time.perf_counter() - t1
        appended += int(new.shape[1])
        if first is None:
            first = t_open + t_dec + t_a
        rows.append(dict(chunk=k, codes_so_far=appended, new_codes=int(new.shape[1]), decode_ms=1e3 * t_dec, session_ms=1e3 * t_a))
        k += 1
        t_prev = time.perf_counter()
    sess.close()
    codes = torch.cat(all_codes, dim=1)
    for r in rows:                                           # (b) the one-shot pass over all codes so far
        n = r["codes_so_far"]
        sync()
        t1 = time.perf_counter()
        m.forward_latent(lconds, text, tl, codes[:, :n], torch.full((B,), n))
        sync()
        r["oneshot_ms"] = 1e3 * (time.perf_counter() - t1)
    return dict(B=B, first_chunk_ms=1e3 * first, session_open_ms=1e3 * t_open, chunks=rows)


os.makedirs(out_dir, exist_ok=True)
results = []
for B in Bs:
    stream(B)                                                # warm-up: code objects, decode graphs, allocator
    r = stream(B)
    results.append(r)
    print(f"B={B:3d} budget {max_codes} chunk {chunk}/{overlap}: first chunk (prefill + {chunk} steps + latents, session open {r['session_open_ms']:.1f} ms "
          f"included) {r['first_chunk_ms']:.1f} ms", flush=True)
    for c in r["chunks"]:
        print(f"   chunk {c['chunk']:2d}: {c['codes_so_far']:4d} codes so far, +{c['new_codes']:3d}: decode {c['decode_ms']:7.1f} ms | latents: session "
              f"{c['session_ms']:6.2f} ms, one-shot over all codes {c['oneshot_ms']:7.2f} ms", flush=True)
with open(os.path.join(out_dir, "stream_v2_bench.json"), "w") as f:
    json.dump(dict(model="24 x 1280 x 20 heads, 34 conditioning tokens, 128 text tokens, bf16", max_codes=max_codes, chunk=chunk, overlap=overlap,
                   results=results), f, indent=1)
