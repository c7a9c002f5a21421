"""bench.py's own multi-rank launcher on CPU: `python bench.py --gpus 2 --engine stub` re-executes itself under
torch.distributed.run with two gloo ranks, shards the batch (strong scaling), broadcasts the speaker bundle, gathers the
waveforms on rank 0 and prints ONE JSON line.  The engine is a labelled stub -- the point is the harness around it."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--engine", "stub", "--steps", "2", "--warmup", "1",
                        "--gen-tokens", "8", "--text-tokens", "16"] + extra, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout            # stdout carries exactly one line
    return json.loads(lines[0])


def test_two_ranks_strong_scaling():
    j = _run(["--gpus", "2", "--utts", "6"])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["engine"] == "stub"
    assert j["config"]["global_batch"] == 6 and j["config"]["per_gpu_batch"] == 3
    assert j["config"]["parallelism"] == "utterance-dp2"
    assert j["stub_rows_ok"] is True
    assert j["steps"] == 2 and j["warmup"] == 1 and j["value"] > 0
    assert j["metric"].startswith("STUB")       # can never be mistaken for a measurement


def test_two_ranks_weak_scaling_and_single_rank():
    j = _run(["--gpus", "2", "--utts", "3", "--weak"])
    assert j["n_gpus"] == 2 and j["scaling"] == "weak" and j["config"]["global_batch"] == 6 and j["stub_rows_ok"] is True
    j1 = _run(["--gpus", "1", "--utts", "5"])
    assert j1["n_gpus"] == 1 and j1["config"]["global_batch"] == 5 and j1["config"]["per_gpu_batch"] == 5 and j1["stub_rows_ok"] is True


def test_eight_ranks_uneven_shares():
    """The real rank count of the metric's last point: 8 gloo ranks, 13 utterances -> shares of 2 and 1 (uneven gather), and the BASELINE split
    64 -> 8 per rank; every utterance reaches rank 0 in utterance order."""
    j = _run(["--gpus", "8", "--utts", "13"])
    assert j["n_gpus"] == 8 and j["scaling"] == "strong" and j["config"]["global_batch"] == 13
    assert j["config"]["per_gpu_batch"] == 2 and j["stub_rows_ok"] is True and j["config"]["parallelism"] == "utterance-dp8"
    j = _run(["--gpus", "8", "--utts", "64"])
    assert j["config"]["per_gpu_batch"] == 8 and j["stub_rows_ok"] is True


def test_lpt_sharding_at_eight_ranks():
    """`shard_utterances` with ragged lengths at world size 8: a partition of all utterances, deterministic, and balanced to within the longest
    utterance (the LPT bound) -- what keeps the ranks of a ragged batch finishing together."""
    import random
    from indextts_amd import dist as D
    rnd = random.Random(5)
    lengths = [rnd.randint(20, 128) for _ in range(64)]
    shares = [D.shard_utterances(64, r, 8, lengths=lengths) for r in range(8)]
    assert sorted(i for sh in shares for i in sh) == list(range(64))
    loads = [sum(lengths[i] for i in sh) for sh in shares]
    assert max(loads) - min(loads) <= max(lengths)
    assert shares == [D.shard_utterances(64, r, 8, lengths=lengths) for r in range(8)]
    assert [len(D.shard_utterances(64, r, 8, lengths=[128] * 64)) for r in range(8)] == [8] * 8


def test_world_size_mismatch_is_an_error():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--engine", "stub", "--gpus", "4"], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_overlapped_steps_two_ranks():
    """`--overlap`: the two-stage software pipeline (decode of step k + 1 on a worker thread, render of step k on the main thread; collectives
    only from the main thread) delivers the same rows as the sequential loop, on one rank and on two."""
    j = _run(["--gpus", "2", "--utts", "6", "--overlap"])
    assert j["n_gpus"] == 2 and j["stub_rows_ok"] is True and j["config"]["step_overlap"] is True and j["steps"] == 2
    j1 = _run(["--gpus", "1", "--utts", "5", "--overlap"])
    assert j1["stub_rows_ok"] is True and j1["config"]["step_overlap"] is True


def test_dump_outputs_same_arrays_run_to_run(tmp_path):
    """`--dump-outputs DIR`: the waveforms the last timed step gathered on rank 0, as float32 .npy, identical from run to run with the same
    arguments (seeded inputs) and on one rank or two (the same utterances, sharded)."""
    import numpy as np
    dumps = []
    for i, gpus in enumerate(["1", "1", "2"]):
        d = tmp_path / f"run{i}"
        j = _run(["--gpus", gpus, "--utts", "6", "--dump-outputs", str(d)])
        assert j["stub_rows_ok"] is True and j["steps"] == 2 and j["ms_per_step"] > 0
        assert j["dumped_outputs"]["arrays"]["waveform"] == [6, j["config"]["mel_frames"] * 256]
        w, cols = np.load(d / "waveform.npy"), np.load(d / "waveform_columns.npy")
        assert w.dtype == np.float32 and cols.dtype == np.float64 and w.shape == (6, cols.size)
        dumps.append((w, cols))
    for w, cols in dumps[1:]:
        assert np.array_equal(w, dumps[0][0]) and np.array_equal(cols, dumps[0][1])


def test_dump_outputs_sample_stays_under_budget(tmp_path, monkeypatch):
    """Over the byte budget, every row is kept at a fixed seeded, sorted set of columns, and the values are the output's own."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_WAVE_BYTES", 4 * 3 * 1000)
    g = torch.Generator().manual_seed(3)
    wav = torch.randint(-32767, 32768, (3, 50000), generator=g, dtype=torch.int32).to(torch.int16)
    shapes = bench.dump_outputs(str(tmp_path / "a"), wav)
    bench.dump_outputs(str(tmp_path / "b"), wav)
    w, cols = np.load(tmp_path / "a" / "waveform.npy"), np.load(tmp_path / "a" / "waveform_columns.npy")
    assert shapes == {"waveform": [3, 1000], "waveform_columns": [1000]} and w.nbytes <= 4 * 3 * 1000
    assert np.all(np.diff(cols) > 0) and cols[0] >= 0 and cols[-1] < 50000
    assert np.array_equal(w, wav.numpy()[:, cols.astype(np.int64)].astype(np.float32))
    assert np.array_equal(cols, np.load(tmp_path / "b" / "waveform_columns.npy"))


def test_full_option_selects_nothing_the_headline_needs():
    """`--full` adds measurements that take runs of their own after the timed steps; the headline's fields are the same with and without it
    (the stub engine has no such legs: only the option and the harness around them are exercised here)."""
    plain, full = _run(["--gpus", "1", "--utts", "5"]), _run(["--gpus", "1", "--utts", "5", "--full"])
    assert sorted(plain) == sorted(full)
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "config"):
        assert plain[k] == full[k], k
    assert full["stub_rows_ok"] is True and full["ms_per_step"] > 0


def test_steps_must_be_positive():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--engine", "stub", "--steps", "0"], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode != 0 and "--steps" in r.stderr
