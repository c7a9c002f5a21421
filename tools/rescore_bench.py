"""GPU box: what the teacher-forced rescoring pass (UnifiedVoice.rescore, itts_gpt_rescore) costs beside the decode it follows -- the
production GPT shape of tools/alignment_bench.py (bf16, 128 text tokens), a 3-beam beam-sample decode of n-gen tokens (the reference's default
mode, hipGraph) and then ONE rescoring pass over its result: scores only, and with 4 (layer, head) pairs, every pair in a layer of its own, at
several chunk sizes.  The variants ALTERNATE inside one process, round after round; the figure per variant is the least of its rounds of
wall time around the call (torch.cuda.synchronize on both sides), next to the decode's own prefill + decode time (itts_gpt_last_timing).
The log-probabilities of all chunk sizes are compared with the first one's (max |d| printed, not asserted: the chunk size changes which GEMM
kernels run).

usage: rescore_bench.py [--rounds 3] [--n-gen 560] [--rows 1,8] [--chunks 32,128,512] [--beams 3]"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n-gen", type=int, default=560)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--chunks", default="32,128,512")
    ap.add_argument("--beams", type=int, default=3)
    a = ap.parse_args()
    import torch
    from indextts_amd import gpt, synth
    from tools.alignment_bench import pairs_of
    gcfg = dict(synth.GPT_V25)
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", **gcfg, precision="bf16", device="cuda:0")
    m.load_state_dict(synth.gpt_weights(gcfg, seed=1234, suppress_eos=True))
    m.post_init_gpt2_config(kv_cache=True, half=True)
    g = torch.Generator().manual_seed(0)
    style = torch.randn(1, 192, generator=g).cuda()
    emo = (torch.randn(1, 1280, generator=g) * 0.1).cuda()
    base = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.8, num_beams=a.beams, repetition_penalty=10.0, length_penalty=0.0)
    pairs = pairs_of(4, gcfg["layers"], gcfg["heads"])
    chunks = [int(v) for v in a.chunks.split(",")]
    variants = [(c, k) for c in chunks for k in (0, 4)]
    for B in [int(v) for v in a.rows.split(",")]:
        text = torch.randint(2, 12000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
        langs = torch.full((B,), 3, dtype=torch.long).cuda()
        cond = dict(langs=langs, emo_vec=emo, campplus_embedding=style)
        decode, got, first_lp, worst = [], {v: [] for v in variants}, None, 0.0
        for rnd in range(a.rounds + 1):                      # round 0 warms up (graph capture, workspace allocation) and is not timed
            codes, _ = m.inference_speech(None, text, max_generate_length=a.n_gen, seed=7, **cond, **base)
            if rnd:
                decode.append(m.last_timing["prefill_ms"] + m.last_timing["decode_ms"])
            for c, k in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ts, al = m.inference_speech_rescore(None, text, codes, alignment_heads=pairs if k else None, chunk=c, **cond)
                torch.cuda.synchronize()
                if rnd:
                    got[(c, k)].append(1e3 * (time.perf_counter() - t0))
                first_lp = ts.logp_model.clone() if first_lp is None else first_lp
                worst = max(worst, float((ts.logp_model - first_lp).abs().max()))
        n = int(codes.shape[1])
        print(f"RESULT B={B} beams={a.beams} decode_ms={min(decode):.2f} ({n} tokens, {min(decode) / n:.4f} ms/token)", flush=True)
        for (c, k), v in got.items():
            print(f"RESULT B={B} chunk={c} pairs={k} rescore_ms={min(v):.2f} rounds=[{', '.join(f'{x:.2f}' for x in v)}] "
                  f"vs_decode={100 * min(v) / min(decode):.2f}%", flush=True)
        print(f"B={B}: mean logp of the rescored codes {ts.mean_logprob().tolist()[:4]}; max |logp - first variant's| over chunk sizes and rounds {worst:.3e}",
              flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
