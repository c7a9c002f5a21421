"""GPU box: what per-token log-probabilities (generate(..., token_scores=True)) cost the GPT decode step -- ms/token (bf16, sampled, num_beams = 1,
hipGraph, the production shape of tools/decode_bench.py) at 1, 8 and 64 rows for three variants: the PARENT commit's library, this library
with scores off, this library with scores on.  Parent and new alternate in FRESH processes on one box (as profiles/r08a did), so the parent's
own run-to-run spread is measured in the same alternation; the scores-off figure is to be judged against that spread.

usage: token_scores_bench.py --parent <tree of the parent commit, built> [--rounds 3] [--n-gen 560] [--rows 1,8,64]
       (the parent tree: `git worktree add <dir> <parent>` and build it there; only its indextts_amd/ is imported)
       token_scores_bench.py --worker --root <tree> --scores 0|1 ...     one variant, one process (what the driver starts)"""
import argparse
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def worker(root: str, scores: bool, n_gen: int, rows):
    sys.path.insert(0, root)
    import torch
    from indextts_amd import gpt, synth
    assert os.path.abspath(os.path.dirname(gpt.__file__)).startswith(os.path.abspath(root)), "the package must come from --root"
    gcfg = dict(synth.GPT_V25)
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", **gcfg, precision="bf16", device="cuda:0")
    m.load_state_dict(synth.gpt_weights(gcfg, seed=1234, suppress_eos=True))
    m.post_init_gpt2_config(kv_cache=True, half=True)
    g = torch.Generator().manual_seed(0)
    style = torch.randn(1, 192, generator=g).cuda()
    emo = (torch.randn(1, 1280, generator=g) * 0.1).cuda()
    kw = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.8, num_beams=1, repetition_penalty=10.0, length_penalty=0.0)
    if scores:
        kw["token_scores"] = True
    for B in rows:
        text = torch.randint(2, 12000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
        langs = torch.full((B,), 3, dtype=torch.long).cuda()
        best = None
        for rep in range(4):                             # the first call captures the step graph
            codes, _ = m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=n_gen, seed=7, **kw)
            t = m.last_timing
            ms = t["decode_ms"] / max(1, t["steps"] - 1)
            best = ms if best is None or (rep > 0 and ms < best) else best
        digest = int(codes.sum().item())
        mean = ""
        if scores:
            mean = f" mean logp_model {float(m.last_scores.mean_logprob().mean()):.4f}"
        print(f"RESULT B={B} ms_per_token={best:.5f} steps={t['steps']} ids_sum={digest}{mean}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n-gen", type=int, default=560)
    ap.add_argument("--rows", default="1,8,64")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=os.path.join(HERE, ".."))
    ap.add_argument("--scores", type=int, default=0)
    a = ap.parse_args()
    rows = [int(v) for v in a.rows.split(",")]
    if a.worker:
        return worker(os.path.abspath(a.root), bool(a.scores), a.n_gen, rows)
    if not a.parent:
        ap.error("--parent <built tree of the parent commit> is required")
    variants = [("parent", os.path.abspath(a.parent), 0), ("new, scores off", os.path.abspath(os.path.join(HERE, "..")), 0),
                ("new, scores on", os.path.abspath(os.path.join(HERE, "..")), 1)]
    got = {name: {B: [] for B in rows} for name, _, _ in variants}
    ids = {}
    for rnd in range(a.rounds):
        for name, root, scores in variants:
            print(f"== {name} run {rnd + 1}", flush=True)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--scores", str(scores), "--n-gen", str(a.n_gen),
                                "--rows", a.rows], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
            print(p.stdout, end="", flush=True)
            if p.returncode != 0:
                print(f"{name}: the worker ended with status {p.returncode}; stopping", flush=True)
                return p.returncode
            for mt in re.finditer(r"RESULT B=(\d+) ms_per_token=([0-9.]+) steps=\d+ ids_sum=(-?\d+)", p.stdout):
                got[name][int(mt.group(1))].append(float(mt.group(2)))
                ids.setdefault(int(mt.group(1)), set()).add(int(mt.group(3)))
    print("== summary: ms/token, median of the runs [min .. max]; vs parent = median / parent median - 1")
    med = lambda v: sorted(v)[len(v) // 2]
    for B in rows:
        base = med(got["parent"][B])
        spread = (max(got["parent"][B]) - min(got["parent"][B])) / base * 100
        for name, _, _ in variants:
            v = got[name][B]
            print(f"B={B:3d} {name:16s}: {med(v):.4f} [{min(v):.4f} .. {max(v):.4f}]  {100 * (med(v) / base - 1):+.2f} % vs parent"
                  + (f"  (parent's own spread {spread:.2f} %)" if name == "parent" else ""))
        print(f"B={B:3d} ids identical across all variants and runs: {len(ids[B]) == 1}")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
