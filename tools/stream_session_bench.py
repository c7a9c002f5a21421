"""Streaming session against consecutive `infer_stream` batches of the same requests (production widths, synthetic weights, EOS suppressed as
in bench.py): N single-segment requests over V voices arrive `--arrival-ms` apart; every voice has its own sampling settings and its own
`max_mel_tokens` (streams of different lengths).

  --leg session   ONE `IndexTTS2.stream_session` over `--slots` slots: a request is submitted when it arrives and starts as soon as a slot is free
  --leg batches   consecutive `infer_stream` calls: whenever the engine is idle, the requests that have arrived for the voice of the oldest
                  waiting request (at most `--slots`) run as one closed batch, which drains to its slowest row before the next one starts

One leg per process (run the two alternately, each under its own time limit); prints one JSON line: time to first audio per request (median,
worst; from the request's arrival), audio seconds per wall second, and for the session the rows per render.  `--out FILE` appends that line."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.mixed_batch_bench import SR, TokenFrontend      # noqa: E402


def build(args):
    from indextts_amd import bigvgan, codec, gpt, infer_v2_5, s2mel, synth
    dev = torch.device("cuda:0")
    gcfg = dict(synth.GPT_V25)
    model = gpt.UnifiedVoice(**gcfg, spk_cond_mode="campplus", precision=args.precision, device=str(dev))
    model.load_state_dict(synth.gpt_weights(gcfg, seed=1234, suppress_eos=True))
    model.post_init_gpt2_config(kv_cache=True, half=args.precision == "bf16")
    bh = dict(synth.BIGVGAN_V2_22K)
    voc = bigvgan.BigVGAN(bh, device=dev, conv_mode="bf16x3")
    voc.load_state_dict(synth.bigvgan_weights(bh, seed=1234))
    voc.to(dev)
    cd = codec.EnhancedCodec(**synth.CODEC_V2, device=dev)
    cd.load_state_dict(synth.codec_weights(seed=1234))
    s2 = s2mel.MyModel(dict(synth.S2MEL_V2, length_regulator=synth.REGULATOR_V2), precision=args.s2mel_precision, device=dev)
    s2.models["cfm"].load_state_dict(synth.s2mel_weights(seed=1234))
    s2.models["length_regulator"].load_state_dict(synth.regulator_weights(seed=1234))
    fe = TokenFrontend(dev, int(gcfg["model_dim"]), args.prompt_frames)
    return infer_v2_5.IndexTTS2(cfg={"gpt": {"stop_mel_token": 8193}, "version": 2.5}, device=str(dev), frontend=fe, gpt=model, bigvgan=voc,
                                semantic_codec=cd, s2mel=s2, codes_to_mel="engine")


def run_session(tts, reqs, arrive, args):
    """-> (first-audio time per request, seconds of audio, wall seconds, rows per render)"""
    first, samples, nxt, ids = [None] * len(reqs), 0, 0, {}
    with tts.stream_session(slots=args.slots, chunk_size=args.chunk, overlap_size=args.overlap, max_mel_tokens=args.gen_tokens,
                            max_text_tokens_per_segment=args.text_tokens, poll_steps=args.poll_steps) as sess:
        t0 = time.perf_counter()
        while nxt < len(reqs) or sess.active:
            now = time.perf_counter() - t0
            while nxt < len(reqs) and arrive[nxt] <= now:
                ids[sess.submit(reqs[nxt])] = nxt
                nxt += 1
            if not sess.active:
                time.sleep(max(0.0, arrive[nxt] - now))
                continue
            for sid, _, pcm, _, _ in sess.step():
                if pcm is not None:
                    samples += len(pcm)
                    if first[ids[sid]] is None:
                        first[ids[sid]] = time.perf_counter() - t0 - arrive[ids[sid]]
        torch.cuda.synchronize()
        return first, samples / SR, time.perf_counter() - t0, list(sess.stats["render_rows"])


def run_batches(tts, reqs, arrive, args):
    first, samples, waiting, nxt = [None] * len(reqs), 0, [], 0
    t0 = time.perf_counter()
    while nxt < len(reqs) or waiting:
        now = time.perf_counter() - t0
        while nxt < len(reqs) and arrive[nxt] <= now:
            waiting.append(nxt)
            nxt += 1
        if not waiting:
            time.sleep(max(0.0, arrive[nxt] - now))
            continue
        voice = reqs[waiting[0]]["spk_audio_prompt"]
        batch = [i for i in waiting if reqs[i]["spk_audio_prompt"] == voice][: args.slots]
        waiting = [i for i in waiting if i not in batch]
        kw = {k: v for k, v in reqs[batch[0]].items() if k not in ("spk_audio_prompt", "text", "lang")}      # a voice's requests share them
        for _, audio, _ in tts.infer_stream(voice, [reqs[i]["text"] for i in batch], "en", chunk_size=args.chunk, overlap_size=args.overlap,
                                            max_text_tokens_per_segment=args.text_tokens, cfm_noise="request", **kw):
            for i, pcm in zip(batch, audio):
                if pcm is not None:
                    samples += len(pcm)
                    if first[i] is None:
                        first[i] = time.perf_counter() - t0 - arrive[i]
    torch.cuda.synchronize()
    return first, samples / SR, time.perf_counter() - t0, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["session", "batches"])
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--voices", type=int, default=4)
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--arrival-ms", type=float, default=250.0, help="request i arrives i x this after the start")
    ap.add_argument("--text-tokens", type=int, default=100)
    ap.add_argument("--gen-tokens", type=int, default=560, help="the longest voice's max_mel_tokens; the others get down to half of it")
    ap.add_argument("--chunk", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=20)
    ap.add_argument("--poll-steps", type=int, default=8)
    ap.add_argument("--prompt-frames", type=int, default=517)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--s2mel-precision", default="fp32x3")
    ap.add_argument("--reps", type=int, default=1, help="timed runs after the warm one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tts = build(args)
    g = torch.Generator().manual_seed(77)
    V = args.voices
    settings = [dict(temperature=0.6 + 0.1 * v, top_p=0.6 + 0.05 * v, top_k=10 + 5 * v, repetition_penalty=2.0 + v, seed=100 + v,
                     max_mel_tokens=int(args.gen_tokens * (1.0 - 0.5 * v / max(1, V - 1)))) for v in range(V)]
    reqs = []
    for i in range(args.requests):
        text = " ".join(str(int(t)) for t in torch.randint(2, 12000, (args.text_tokens,), generator=g))
        reqs.append(dict(spk_audio_prompt=f"voice{i % V}.wav", text=text, lang="en", **settings[i % V]))      # arrival order interleaves the voices
    arrive = [i * args.arrival_ms / 1000.0 for i in range(len(reqs))]
    leg = run_session if args.leg == "session" else run_batches
    runs = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(1 + args.reps):                             # run 0 warms graphs, workspaces and caches
            res = leg(tts, reqs, arrive, args)
            if k:
                runs.append(res)
    line = dict(leg=args.leg, requests=len(reqs), voices=V, slots=args.slots, arrival_ms=args.arrival_ms, chunk=args.chunk, overlap=args.overlap,
                poll_steps=args.poll_steps if args.leg == "session" else None, gen_tokens=[s["max_mel_tokens"] for s in settings],
                first_audio_median_s=[round(statistics.median(r[0]), 4) for r in runs], first_audio_worst_s=[round(max(r[0]), 4) for r in runs],
                audio_seconds=[round(r[1], 2) for r in runs], wall_seconds=[round(r[2], 3) for r in runs],
                audio_seconds_per_sec=[round(r[1] / r[2], 2) for r in runs],
                rows_per_render_mean=[round(sum(r[3]) / len(r[3]), 2) for r in runs] if args.leg == "session" else None)
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
