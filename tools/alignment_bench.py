"""GPU box: what the text-attention export (generate(..., alignment_heads=)) costs the GPT decode step -- ms/token (bf16, sampled, num_beams = 1,
hipGraph, the production shape of tools/decode_bench.py and tools/token_scores_bench.py) at 1, 8 and 64 rows with the export off and with
1, 4 and 8 (layer, head) pairs, every pair in a layer of its own (the costliest placement: one extra launch per pair).  The variants ALTERNATE
inside one process, round after round, so drift of the box hits them alike; the figure per variant is the least of its rounds, next to the
spread of the off variant's rounds.  The generated ids must be the same in every variant and round (asserted with torch.equal against the
first call's).

"Off costs nothing" is a comparison with the PARENT commit's library, which this process cannot hold: with --parent <built tree of the parent
commit> the tool also alternates fresh processes of the parent and of this tree with the export off (as tools/token_scores_bench.py does;
across processes the ids are compared by their printed sum).

usage: alignment_bench.py [--rounds 3] [--n-gen 560] [--rows 1,8,64] [--pairs 0,1,4,8] [--parent <tree>]
       alignment_bench.py --worker --root <tree> ...      one process over the variants (what the driver starts for --parent)"""
import argparse
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def pairs_of(k: int, layers: int, heads: int):
    """k pairs, each in another layer, spread over the stack; heads cycle"""
    return [((2 * i + 1) * layers // (2 * k), (7 * i + 3) % heads) for i in range(k)]


def worker(root: str, n_gen: int, rows, pair_counts, rounds: int):
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
    base = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.8, num_beams=1, repetition_penalty=10.0, length_penalty=0.0)
    for B in rows:
        text = torch.randint(2, 12000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
        langs = torch.full((B,), 3, dtype=torch.long).cuda()
        got = {k: [] for k in pair_counts}
        digest = {}
        first_codes = None
        for rnd in range(rounds + 1):                        # round 0 captures every variant's step graph and is not timed
            for k in pair_counts:
                kw = dict(base, alignment_heads=pairs_of(k, gcfg["layers"], gcfg["heads"])) if k else base
                codes, _ = m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=n_gen, seed=7, **kw)
                t = m.last_timing
                if rnd:
                    got[k].append(t["decode_ms"] / max(1, t["steps"] - 1))
                digest.setdefault(k, set()).add(int(codes.sum().item()))      # (printed: what the --parent driver compares across processes)
                if first_codes is None:
                    first_codes = codes.clone()
                assert torch.equal(codes, first_codes), f"B={B}: the ids of {k} pairs (round {rnd}) differ from the first variant's"
                if k:
                    al = m.last_alignment
                    mass = float(al.attn[:, 1:int(al.lengths.min())].sum(-1).mean())
        off = got[pair_counts[0]]
        for k in pair_counts:
            v = got[k]
            print(f"RESULT B={B} pairs={k} ms_per_token={min(v):.5f} rounds=[{', '.join(f'{x:.4f}' for x in v)}] steps={t['steps']} "
                  f"vs_first={100 * (min(v) / min(off) - 1):+.2f}% ids_sum={next(iter(digest[k]))}", flush=True)
        print(f"B={B}: ids identical across the variants; spread of the first variant's rounds {100 * (max(off) - min(off)) / min(off):.2f} %; "
              f"mean text mass of an exported row (last variant) {mass if pair_counts[-1] else float('nan'):.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n-gen", type=int, default=560)
    ap.add_argument("--rows", default="1,8,64")
    ap.add_argument("--pairs", default="0,1,4,8")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=os.path.join(HERE, ".."))
    a = ap.parse_args()
    rows, pair_counts = [int(v) for v in a.rows.split(",")], [int(v) for v in a.pairs.split(",")]
    if a.worker or not a.parent:
        return worker(os.path.abspath(a.root), a.n_gen, rows, pair_counts, a.rounds)
    here = os.path.abspath(os.path.join(HERE, ".."))
    variants = [("parent", os.path.abspath(a.parent)), ("new, export off", here)]
    got = {name: {B: [] for B in rows} for name, _ in variants}
    ids = {}
    for rnd in range(a.rounds):
        for name, root in variants:
            print(f"== {name} run {rnd + 1}", flush=True)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--pairs", "0", "--rounds", "2", "--n-gen", str(a.n_gen),
                                "--rows", a.rows], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
            print(p.stdout, end="", flush=True)
            if p.returncode != 0:
                print(f"{name}: the worker ended with status {p.returncode}; stopping", flush=True)
                return p.returncode
            for mt in re.finditer(r"RESULT B=(\d+) pairs=0 ms_per_token=([0-9.]+) .* ids_sum=(-?\d+)", p.stdout):
                got[name][int(mt.group(1))].append(float(mt.group(2)))
                ids.setdefault(int(mt.group(1)), set()).add(int(mt.group(3)))
    print("== summary: ms/token, median of the runs [min .. max]; vs parent = median / parent median - 1")
    med = lambda v: sorted(v)[len(v) // 2]
    for B in rows:
        basev = med(got["parent"][B])
        spread = (max(got["parent"][B]) - min(got["parent"][B])) / basev * 100
        for name, _ in variants:
            v = got[name][B]
            print(f"B={B:3d} {name:16s}: {med(v):.4f} [{min(v):.4f} .. {max(v):.4f}]  {100 * (med(v) / basev - 1):+.2f} % vs parent"
                  + (f"  (parent's own spread {spread:.2f} %)" if name == "parent" else ""))
        print(f"B={B:3d} ids identical across both libraries and all runs: {len(ids[B]) == 1}")
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
