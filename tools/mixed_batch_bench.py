"""Mixed-request batch against what same-voice grouping can do with the same requests (production widths, synthetic weights, EOS
suppressed as in bench.py): 64 single-segment requests over 8 voices, every voice with its own sampling settings, num_beams = 1 by
default.  `--num-beams 3 --beam-settings own` measures the reference's default 3-beam mode with per-request settings (the beam kernels'
per-group table); the grouped leg is the same in both modes (its calls carry one set of settings each).

  --leg mixed     ONE `IndexTTS2.infer_requests` call over the 64 requests
  --leg grouped   8 `infer_batch` calls of 8 (one per voice, its settings as the call's) -- the widest batches the serving shell could
                  form before per-row voices and per-row sampling settings

One leg per process (run the two alternately, each under its own time limit); prints one JSON line with the wall time of a warm call and
the audio seconds it produced.  `--out FILE` appends that line to a file."""
import argparse
import json
import os
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR = 22050


class TokenFrontend:
    """prompt / text stages of the benchmark: seeded random bundles per voice name, a text is a string of token ids"""

    def __init__(self, dev, model_dim, prompt_frames):
        self.dev, self.D, self.prompt_frames = dev, model_dim, prompt_frames

    def speaker_bundle(self, name):
        g = torch.Generator().manual_seed(1000 + sum(map(ord, str(name))))
        fp = self.prompt_frames - 16 * (sum(map(ord, str(name))) % 4)              # prompts of different lengths
        return dict(style=torch.randn(1, 192, generator=g).to(self.dev), spk_cond_emb=torch.zeros(1, 4, 1024, device=self.dev),
                    ref_mel=(torch.randn(1, 80, fp, generator=g) * 2 - 4).to(self.dev),
                    prompt_condition=torch.randn(1, fp, 512, generator=g).to(self.dev))

    def emo_cond(self, name):
        return torch.zeros(1, 4, 1024, device=self.dev)

    def merge_emovec(self, spk_cond_emb, emo_cond_emb, alpha):
        return (torch.randn(1, self.D, generator=torch.Generator().manual_seed(6)) * 0.1 * float(alpha)).to(self.dev)

    def text_segments(self, text, lang, max_text_tokens_per_segment, text_normalization, capacity):
        return [torch.tensor([int(v) for v in text.split()] + [1], dtype=torch.int32)]

    def lang_id(self, lang):
        return 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["mixed", "grouped"])
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--voices", type=int, default=8)
    ap.add_argument("--text-tokens", type=int, default=128)
    ap.add_argument("--gen-tokens", type=int, default=560)
    ap.add_argument("--prompt-frames", type=int, default=517)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--s2mel-precision", default="fp32x3")
    ap.add_argument("--num-beams", type=int, default=1)
    ap.add_argument("--beam-settings", default="shared", choices=["shared", "own"],
                    help="num_beams > 1, mixed leg: 'own' keeps every request's settings (infer_requests(beam_settings='own')); 'shared' is "
                         "refused for requests whose settings differ")
    ap.add_argument("--reps", type=int, default=1, help="timed calls after the warm one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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
    tts = infer_v2_5.IndexTTS2(cfg={"gpt": {"stop_mel_token": 8193}, "version": 2.5}, device=str(dev), frontend=fe, gpt=model, bigvgan=voc,
                               semantic_codec=cd, s2mel=s2, codes_to_mel="engine")
    g = torch.Generator().manual_seed(77)
    per_voice = args.requests // args.voices
    settings = [dict(temperature=0.6 + 0.1 * v, top_p=0.6 + 0.05 * v, top_k=10 + 5 * v, repetition_penalty=2.0 + v, seed=100 + v)
                for v in range(args.voices)]
    reqs = []
    for i in range(per_voice * args.voices):
        v = i % args.voices                                                        # arrival order interleaves the voices
        text = " ".join(str(int(t)) for t in torch.randint(2, 12000, (args.text_tokens,), generator=g))
        reqs.append(dict(spk_audio_prompt=f"voice{v}.wav", text=text, lang="en", **settings[v]))
    wide = dict(num_beams=args.num_beams, max_mel_tokens=args.gen_tokens)
    mixed_kw = dict(beam_settings=args.beam_settings) if args.num_beams > 1 else {}

    def run():
        if args.leg == "mixed":
            return tts.infer_requests(reqs, **wide, **mixed_kw)
        outs = [None] * len(reqs)
        for v in range(args.voices):
            idx = [i for i in range(len(reqs)) if i % args.voices == v]
            res = tts.infer_batch(f"voice{v}.wav", [reqs[i]["text"] for i in idx], "en", **settings[v], **wide)
            for i, o in zip(idx, res):
                outs[i] = o
        return outs

    times, audio = [], 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                            # max_mel_tokens overflow: EOS is suppressed
        for k in range(1 + args.reps):                             # call 0 warms graphs, workspaces and caches
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = run()
            torch.cuda.synchronize()
            if k:
                times.append(time.perf_counter() - t0)
            audio = sum(o[1].shape[0] for o in outs) / SR
    best = min(times)
    line = dict(leg=args.leg, num_beams=args.num_beams, beam_settings=args.beam_settings if args.num_beams > 1 else None, requests=len(reqs), voices=args.voices, text_tokens=args.text_tokens, gen_tokens=args.gen_tokens,
                seconds=[round(t, 4) for t in times], audio_seconds=round(audio, 2), audio_seconds_per_sec=round(audio / best, 2),
                stage_seconds_last_call={k: round(float(v), 4) for k, v in tts.last_timing.items()})
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
