#!/usr/bin/env python
"""What the delivery stage costs: the tail of `infer_requests` after the vocoder, and a stream render's rows-to-events time.

Workload (synthetic vocoder output, so that only the tail is timed): 64 requests of about 22 s -- two segments of 11 s each, 128 rows of one
ragged vocoder batch on the device.  Alternated in ONE process, `--repeats` rounds after `--warmup`:

  host            the tail the pipeline had before delivery formats (and still has without `audio_format`): clamp(32767 x), one `.cpu()` per
                  row, torch.cat of the interval silences on the CPU, `.type(torch.int16)`
  22050/pcm_s16le `output.convert`: assembled, encoded on the device, one device-to-host copy
  48000/pcm_s16le the same through the resampler (L / M = 320 / 147)
  8000/mulaw      the same (L / M = 160 / 441), one byte per sample

and for streams, 8 jobs per render (a `stream_session` of 8 slots), chunks of 100 codes overlapping by 20: from the vocoder's rows on the device
to the pieces on the host -- `RowStream.push` on numpy after one `.cpu()` per row, against `output.deliver`.

`loudness` (`--loudness-only` runs nothing else): 48000/pcm_s16le and 8000/mulaw, each against itself with
`loudness_lufs=-23`, alternated the same way; and the measuring entry and the gain launch on their own.

`limiter` (`--limiter-only` runs nothing else): 48000/pcm_s16le/-23lufs against itself with `-1limit` and with `-1limit/tp`,
alternated the same way; and the limiter launch in both modes and the true-peak meter on their own.

Every timing is a host clock around work that starts after a device synchronise and ends with the data on the host.  Prints one JSON line;
`--out` also writes it to a file.  Nothing is gated on these numbers."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from indextts_amd import output as O                      # noqa: E402
from indextts_amd.streaming import RowStream              # noqa: E402

DEV = "cuda:0"
SIL_MS = 200


def host_tail(wav, lens, groups):
    """the parent commit's tail of infer_requests (indextts_amd/infer_v2_5.py, after `self.bigvgan(...)`)"""
    w = torch.clamp(32767.0 * wav, -32767.0, 32767.0)
    rows = [w[i, :, : lens[i]].cpu() for i in range(w.shape[0])]
    sil = torch.zeros(1, int(22050 * SIL_MS / 1000.0))
    out = []
    for g in groups:
        parts = []
        for k, i in enumerate(g):
            parts.append(rows[i])
            if k < len(g) - 1:
                parts.append(sil)
        out.append((22050, torch.cat(parts, dim=1).type(torch.int16).numpy().T))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, r


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), n=len(ms))


LOUDNESS_FORMATS = ["48000/pcm_s16le", "8000/mulaw"]
LOUDNESS_TARGET = -23.0


def loudness_variant(a, wav, lens, groups):
    """each format against itself with `loudness_lufs`, alternated in this process after warm-up; and the measuring entry (its four launches) and
    the gain launch on their own (a host clock from a synchronise to a synchronise: wrapper, table upload and launches)"""
    cases = {}
    for f in LOUDNESS_FORMATS:
        cases[f] = (lambda f=f: O.convert(wav[:, 0, :], lens, groups, f, SIL_MS))
        cases[f"{f}/{LOUDNESS_TARGET:g}lufs"] = (lambda f=f: O.convert(wav[:, 0, :], lens, groups, f"{f}/{LOUDNESS_TARGET:g}lufs", SIL_MS))
    times = {k: [] for k in cases}
    for it in range(a.warmup + a.repeats):
        for name, fn in cases.items():
            ms, res = timed(fn)
            if it >= a.warmup:
                times[name].append(ms)
    out = dict(target_lufs=LOUDNESS_TARGET, tail={k: summary(v) for k, v in times.items()})
    # the launches alone: 64 sequences of white noise at the delivery rate, as long as the requests are there
    sil = int(22050 * SIL_MS / 1000.0)
    for rate in (48000, 8000):
        L, M, _, _ = O.resample_params(22050, rate)
        ns = [O.resampled_length(sum(lens[i] for i in g) + sil * (len(g) - 1), L, M) for g in groups]
        starts = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        x = (torch.rand(int(starts[-1]), device=DEV) * 2 - 1) * 0.5
        seqs = [(int(s), n) for s, n in zip(starts[:-1], ns)]
        longest = max(range(len(ns)), key=lambda i: ns[i])
        per = {"measure_64_sequences": [], "gain_64_sequences": [], "measure_longest_alone": []}
        for it in range(a.warmup + a.repeats):
            for name, fn in (("measure_64_sequences", lambda: O._measure_seq(x, seqs, rate, True, "bench")),
                             ("measure_longest_alone", lambda: O._measure_seq(x, [seqs[longest]], rate, True, "bench"))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lufs, peak = fn()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    per[name].append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            O.loudness_gain(lufs, LOUDNESS_TARGET, peak, -1.0)
            torch.cuda.synchronize()
            if it >= a.warmup:
                per["gain_64_sequences"].append((time.perf_counter() - t0) * 1e3)
        out[f"launches_{rate}"] = dict(samples=int(starts[-1]), longest_samples=int(ns[longest]), sub_blocks=int(sum(n // O.loudness_hop(rate) for n in ns)),
                                       **{k: summary(v) for k, v in per.items()})
    return out


LIMITER_BASE = "48000/pcm_s16le/-23lufs"


def limiter_variant(a, wav, lens, groups):
    """the loudness format against itself with a limiter line (`-1limit`) and a true-peak line (`-1limit/tp`), alternated in this process after
    warm-up, at the shape of the other variants; and the limiter and the true-peak meter on their own over 64 sequences at 48 kHz"""
    cases = {f: (lambda f=f: O.convert(wav[:, 0, :], lens, groups, f, SIL_MS)) for f in
             (LIMITER_BASE, LIMITER_BASE + "/-1limit", LIMITER_BASE + "/-1limit/tp")}
    times = {k: [] for k in cases}
    for it in range(a.warmup + a.repeats):
        for name, fn in cases.items():
            ms, _ = timed(fn)
            if it >= a.warmup:
                times[name].append(ms)
    out = dict(tail={k: summary(v) for k, v in times.items()})
    rate, sil = 48000, int(22050 * SIL_MS / 1000.0)
    L, M, _, _ = O.resample_params(22050, rate)
    ns = [O.resampled_length(sum(lens[i] for i in g) + sil * (len(g) - 1), L, M) for g in groups]
    starts = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    x = (torch.rand(int(starts[-1]), device=DEV) * 2 - 1) * 0.5
    rows = [(int(s), n, 0, int(s), 0, n, 1) for s, n in zip(starts[:-1], ns)]
    per = {"limiter_64_sequences": lambda: O.limiter_seq(x, rows, rate, 2.0, -1.0, False, int(starts[-1]), stats=True),
           "limiter_true_peak_64_sequences": lambda: O.limiter_seq(x, rows, rate, 2.0, -1.0, True, int(starts[-1]), stats=True),
           "true_peak_meter_64_sequences": lambda: O.true_peak_seq(x, [(r[0], r[1]) for r in rows])}
    alone = {k: [] for k in per}
    for it in range(a.warmup + a.repeats):
        for name, fn in per.items():
            ms, _ = timed(fn)
            if it >= a.warmup:
                alone[name].append(ms)
    out["launches_48000"] = dict(samples=int(starts[-1]), lookahead=O.limiter_lookahead(rate), **{k: summary(v) for k, v in alone.items()})
    return out


def emit(result, path):
    line = json.dumps(result)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=22.0)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loudness-only", action="store_true", help="only the loudness variant (DESIGN section 22)")
    ap.add_argument("--limiter-only", action="store_true", help="only the limiter / true-peak variant (DESIGN section 23)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this meter needs the GPU: a CPU run says nothing about the device stage"
    g = torch.Generator(device=DEV).manual_seed(0)
    seg = int(a.seconds / 2 * 22050) // 256 * 256
    n_rows = 2 * a.requests
    rng = np.random.default_rng(0)
    lens = [seg - 256 * int(v) for v in rng.integers(0, 40, n_rows)]             # ragged, as a vocoder batch is
    wav = (torch.rand(n_rows, 1, seg, device=DEV, generator=g) * 2 - 1) * 0.8
    groups = [[2 * r, 2 * r + 1] for r in range(a.requests)]
    head = dict(tool="output_stage_bench", requests=a.requests, rows=n_rows, audio_seconds=round(sum(lens) / 22050.0, 1), interval_silence_ms=SIL_MS)
    if a.loudness_only:
        emit(dict(head, loudness=loudness_variant(a, wav, lens, groups)), a.out)
        return
    if a.limiter_only:
        emit(dict(head, limiter=limiter_variant(a, wav, lens, groups)), a.out)
        return
    formats = ["22050/pcm_s16le", "48000/pcm_s16le", "8000/mulaw"]
    cases = {"host": lambda: host_tail(wav, lens, groups)}
    for f in formats:
        cases[f] = (lambda f=f: O.convert(wav[:, 0, :], lens, groups, f, SIL_MS))
    times = {k: [] for k in cases}
    for it in range(a.warmup + a.repeats):
        for name, fn in cases.items():                   # alternated: every round runs every case once
            ms, res = timed(fn)
            if it >= a.warmup:
                times[name].append(ms)
            elif it == 0 and name == "22050/pcm_s16le":  # the two 22050 paths agree within 1 LSB (rounding against truncation)
                ref = host_tail(wav, lens, groups)
                worst = max(int(np.abs(x.astype(np.int32) - y[:, 0].astype(np.int32)).max()) for x, (_, y) in zip(res, ref))
                assert worst <= 1, worst
    result = dict(head, tail={k: summary(v) for k, v in times.items()})
    result["loudness"] = loudness_variant(a, wav, lens, groups)
    result["limiter"] = limiter_variant(a, wav, lens, groups)

    # ---- streams: 8 jobs per render --------------------------------------------------------------------------------------------------------
    slots, chunk, overlap, fpc, n_chunks = 8, 100, 20, 2 * 1.72, 6
    samples = int(chunk * fpc) * 256
    rows = [(torch.rand(slots, 1, samples, device=DEV, generator=g) * 2 - 1) * 0.8 for _ in range(n_chunks)]
    stream_times = {}
    for name in ["host"] + formats:
        per_render = []
        for it in range(a.warmup + a.repeats):
            if name == "host":
                st = [RowStream(chunk, overlap, fpc) for _ in range(slots)]
            else:
                ovlp = RowStream(chunk, overlap, fpc).ovlp
                st = [O.OutputStream(name, ovlp) for _ in range(slots)]
            for k, w in enumerate(rows):
                last = k == n_chunks - 1
                if name == "host":
                    ms, _ = timed(lambda: [st[i].push(w[i, 0].float().cpu().numpy(), last) for i in range(slots)])
                else:
                    ms, _ = timed(lambda: O.deliver(st, [w[i, 0] for i in range(slots)], [last] * slots))
                if it >= a.warmup:
                    per_render.append(ms)
        stream_times[name] = summary(per_render)
    result["stream_render_to_events"] = dict(slots=slots, chunk_codes=chunk, overlap_codes=overlap, samples_per_row=samples, per_render=stream_times)
    emit(result, a.out)


if __name__ == "__main__":
    main()
