"""GPU box: what ingesting a code prefix (generate(code_prefix=), itts_gpt_set_code_prefix) costs beside the two things it replaces or
resembles -- the production GPT shape of tools/rescore_bench.py (bf16, 128 text tokens, sampling at num_beams = 1 with hipGraph), 1 and 8
rows, prefixes of k = 280 and 560 codes taken from a plain run of k + tail codes.  Three things are timed in the same process, round after
round, the figure per variant being the least of its rounds:
  ingest   a call with code_prefix = the plain run's first k codes and max_new_tokens = k + 1: prompt prefill + ingest + one selection
           (itts_gpt_last_timing's prefill_ms, which spans both; the plain call's prefill_ms is printed beside it), at prefix_chunk 32 / 128
  decode   the same k codes as plain decode steps: k x the plain run's ms per token (the path this change leaves as it was)
  rescore  UnifiedVoice.rescore over the same k codes at chunk 128: wall time, torch.cuda.synchronize on both sides
Nothing is asserted; whether the continuation equals the plain run's tail is printed (bf16: no claim).

usage: code_prefix_bench.py [--rounds 3] [--ks 280,560] [--rows 1,8] [--chunks 32,128] [--tail 16]"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ks", default="280,560")
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--chunks", default="32,128")
    ap.add_argument("--tail", type=int, default=16)
    a = ap.parse_args()
    import torch
    from indextts_amd import gpt, synth
    gcfg = dict(synth.GPT_V25)
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", **gcfg, precision="bf16", device="cuda:0")
    m.load_state_dict(synth.gpt_weights(gcfg, seed=1234, suppress_eos=True))
    m.post_init_gpt2_config(kv_cache=True, half=True)
    g = torch.Generator().manual_seed(0)
    style = torch.randn(1, 192, generator=g).cuda()
    emo = (torch.randn(1, 1280, generator=g) * 0.1).cuda()
    base = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.8, num_beams=1, repetition_penalty=10.0, seed=7)
    chunks = [int(v) for v in a.chunks.split(",")]
    for B in [int(v) for v in a.rows.split(",")]:
        text = torch.randint(2, 12000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
        cond = dict(langs=torch.full((B,), 3, dtype=torch.long).cuda(), emo_vec=emo, campplus_embedding=style)
        emb, mask, _, _ = m.inference_speech_stream(None, text, **cond)
        for k in [int(v) for v in a.ks.split(",")]:
            total = k + a.tail
            plain_ms, prefill_ms, ingest, rescore, same, passes = [], [], {c: [] for c in chunks}, [], None, {}
            for rnd in range(a.rounds + 1):                  # round 0 warms up (graph capture, workspace allocation) and is not timed
                plain, _ = m.inference_speech(None, text, max_generate_length=total, **cond, **base)
                t = dict(m.last_timing)
                if rnd:
                    plain_ms.append(t["decode_ms"] / max(1, t["steps"] - 1))
                    prefill_ms.append(t["prefill_ms"])
                prefix = plain[:, :k]
                for c in chunks:
                    m.inference_speech(None, text, max_generate_length=k + 1, code_prefix=prefix, prefix_chunk=c, **cond, **base)
                    passes[c] = m.last_prefix["chunks"]
                    if rnd:
                        ingest[c].append(m.last_timing["prefill_ms"])
                cont, _ = m.inference_speech(None, text, max_generate_length=total, code_prefix=prefix, prefix_chunk=chunks[-1], **cond, **base)
                same = bool(torch.equal(cont, plain))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.rescore(emb, mask, prefix, chunk=128)
                torch.cuda.synchronize()
                if rnd:
                    rescore.append(1e3 * (time.perf_counter() - t0))
            print(f"RESULT B={B} k={k} plain_prefill_ms={min(prefill_ms):.2f} decode_ms_per_token={min(plain_ms):.4f} "
                  f"k_decode_steps_ms={k * min(plain_ms):.2f} rescore128_ms={min(rescore):.2f}", flush=True)
            for c in chunks:
                print(f"RESULT B={B} k={k} prefix_chunk={c} prefill_plus_ingest_ms={min(ingest[c]):.2f} "
                      f"ingest_ms={min(ingest[c]) - min(prefill_ms):.2f} passes={passes[c]} "
                      f"rounds=[{', '.join(f'{x:.2f}' for x in ingest[c])}]", flush=True)
            print(f"B={B} k={k}: continuation equals the plain run's tail: {same}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
