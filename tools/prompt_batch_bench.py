"""N cold voice prompts: N serial `EngineFrontend.speaker_bundle` calls against ONE `speaker_bundles` call.

A checkpoint directory with the reference's file layout is written to a temporary directory: w2v-bert-2.0 at its production widths (the 17 layers
below the tapped hidden state), the real CAMPPlus architecture, the production length regulator -- synthetic seeded weights, since only the time is
measured -- and N synthetic WAV prompts of mixed lengths up to 15 s.  After one untimed pass of each leg the two legs run alternately `--rounds`
times in this one process (every call is cold for the caches: the front end has none; only the DSP tables and the allocator are warm), and one JSON
line is printed: per leg the median and the fastest wall time, and their ratio.  `--out FILE` writes that line to a file (profiles/<name>/...).

  python tools/prompt_batch_bench.py --prompts 64 --out profiles/prompt_batch/prompt_batch_n64.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_checkpoint_dir(d, n_prompts, min_seconds, max_seconds, rate, seed):
    from scipy.io import wavfile
    from oracle import campplus_oracle as CO
    from oracle import codec_oracle as KO
    from oracle import w2vbert_oracle as WO
    from tools.make_golden_audio import speechlike
    wcfg = WO.W2VBertCfg(num_hidden_layers=17)                              # the layers below hidden_states[17]
    rcfg = KO.RegulatorConfig()
    wdir = os.path.join(d, "hf_cache", "w2v-bert-2.0")
    os.makedirs(wdir)
    with open(os.path.join(wdir, "config.json"), "w") as f:
        json.dump(dict(hidden_size=wcfg.hidden_size, num_hidden_layers=wcfg.num_hidden_layers, num_attention_heads=wcfg.num_attention_heads,
                       intermediate_size=wcfg.intermediate_size, feature_projection_input_dim=wcfg.feature_projection_input_dim,
                       position_embeddings_type="relative_key", left_max_position_embeddings=wcfg.left_max_position_embeddings,
                       right_max_position_embeddings=wcfg.right_max_position_embeddings,
                       conv_depthwise_kernel_size=wcfg.conv_depthwise_kernel_size, hidden_act="swish", layer_norm_eps=wcfg.layer_norm_eps,
                       add_adapter=False), f)
    torch.save(WO.synth_weights(wcfg, seed=seed), os.path.join(wdir, "pytorch_model.bin"))
    torch.save({"mean": torch.zeros(wcfg.hidden_size), "var": torch.ones(wcfg.hidden_size)}, os.path.join(d, "wav2vec2bert_stats.pt"))
    torch.save(CO.synth_weights(), os.path.join(d, "hf_cache", "campplus_cn_common.bin"))
    rsd = KO.synth_regulator_weights(rcfg, seed + 1)
    torch.save({"net": {"cfm": {"placeholder": torch.zeros(1)}, "length_regulator": rsd}}, os.path.join(d, "s2mel.pth"))
    paths, seconds = [], np.linspace(max_seconds, min_seconds, n_prompts)
    for i, sec in enumerate(seconds):                                       # mixed lengths, longest first and then interleaved
        n = int(round(float(sec) * rate))
        p = os.path.join(d, f"prompt{i:03d}.wav")
        wavfile.write(p, rate, np.round(speechlike(n, rate, seed + 10 + i) * 32767.0).astype(np.int16))
        paths.append(p)
    order = list(range(0, n_prompts, 2)) + list(range(1, n_prompts, 2))
    cfg = {"w2v_stat": "wav2vec2bert_stats.pt", "s2mel_checkpoint": "s2mel.pth",
           "s2mel": {"length_regulator": {"channels": rcfg.channels, "sampling_ratios": [1] * rcfg.n_layers, "is_discrete": False,
                                          "in_channels": rcfg.in_channels, "content_codebook_size": rcfg.codebook_size},
                     "preprocess_params": {"sr": 22050, "spect_params": {"n_fft": 1024, "win_length": 1024, "hop_length": 256, "n_mels": 80,
                                                                         "fmin": 0, "fmax": "None"}}}}
    return cfg, [paths[i] for i in order], [float(seconds[i]) for i in order]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=64)
    ap.add_argument("--min-seconds", type=float, default=3.0)
    ap.add_argument("--max-seconds", type=float, default=15.0)
    ap.add_argument("--rate", type=int, default=24000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=51)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from indextts_amd.frontend import EngineFrontend
    with tempfile.TemporaryDirectory() as d:
        cfg, paths, seconds = write_checkpoint_dir(d, a.prompts, a.min_seconds, a.max_seconds, a.rate, a.seed)
        fe = EngineFrontend(cfg, d, a.device)
        legs = {"serial": lambda: [fe.speaker_bundle(p) for p in paths], "batched": lambda: fe.speaker_bundles(paths)}
        _, ser = timed(legs["serial"])                                       # untimed pass of each leg
        _, bat = timed(legs["batched"])
        diff = max(float((b[k] - s[k]).abs().max()) for b, s in zip(bat, ser) for k in s)
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k in legs:                                                   # alternated on one visit
                times[k].append(timed(legs[k])[0])
    res = dict(tool="prompt_batch_bench", prompts=a.prompts, audio_seconds=round(sum(seconds), 1), rounds=a.rounds,
               serial_s_median=statistics.median(times["serial"]), serial_s_min=min(times["serial"]),
               batched_s_median=statistics.median(times["batched"]), batched_s_min=min(times["batched"]),
               serial_over_batched=statistics.median(times["serial"]) / statistics.median(times["batched"]),
               head_groups=len(fe.campplus.last_head_groups), max_abs_diff_batched_vs_serial=diff,
               device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
