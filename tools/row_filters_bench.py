"""GPU box: what the per-slot filter table costs per decoded token (bf16, sampled, num_beams = 1, hipGraph, production widths) -- the shape of
decode_filters_bench.py.  Four variants alternated in one process: no filter, a table of off entries (what a stream session without filters
runs under), the call-wide record, a full table (every row its own entry);
with --parent DIR (a checkout of the parent commit with its library built) the parent's no-filter call is one more variant of the same
alternation -- its package is imported under another name and its library loaded beside this one's, both on torch's HIP runtime.
usage: row_filters_bench.py [--parent DIR] [--n-gen 300] [--rows 8,64] [--rounds 5] [--json OUT]"""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from indextts_amd import gpt, synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="root of a checkout of the parent commit, library built")
ap.add_argument("--n-gen", type=int, default=300)
ap.add_argument("--rows", default="8,64")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()

FILTERS = dict(min_new_tokens=20, suppress_tokens=[3, 5], min_p=0.05)
OTHER = dict(min_length=200, begin_suppress_tokens=[7], epsilon_cutoff=0.0005)        # the odd rows' entry: a table of two kinds of rows


def load_parent(root):
    pkg = os.path.join(os.path.abspath(root), "indextts_amd")
    spec = importlib.util.spec_from_file_location("indextts_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["indextts_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("indextts_amd_parent.gpt")


def engine(g):
    gcfg = dict(synth.GPT_V25)
    m = g.UnifiedVoice(spk_cond_mode="campplus", **gcfg, precision="bf16", device="cuda:0")
    m.load_state_dict(synth.gpt_weights(gcfg, seed=1234, suppress_eos=True))
    m.post_init_gpt2_config(kv_cache=True, half=True)
    return m


engines = {"own": engine(gpt)}
if args.parent:
    engines["parent"] = engine(load_parent(args.parent))
gen = torch.Generator().manual_seed(0)
style = torch.randn(1, 192, generator=gen).cuda()
emo = (torch.randn(1, 1280, generator=gen) * 0.1).cuda()
kw = dict(do_sample=True, top_p=0.8, top_k=30, temperature=0.8, num_beams=1, repetition_penalty=10.0, length_penalty=0.0)
report = []
for B in [int(v) for v in args.rows.split(",")]:
    text = torch.randint(2, 12000, (B, 128), generator=torch.Generator().manual_seed(B)).cuda()
    langs = torch.full((B,), 3, dtype=torch.long).cuda()
    variants = ([("parent_plain", "parent", {})] if args.parent else []) + [
        ("plain", "own", {}), ("off_table", "own", dict(row_filters=[None] * B)), ("call_wide", "own", FILTERS), ("table", "own", dict(row_filters=[FILTERS if b % 2 == 0 else OTHER for b in range(B)]))]
    best, every = {}, {}
    for rep in range(args.rounds + 1):                       # round 0 warms every graph up
        for name, which, extra in variants:
            m = engines[which]
            m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=args.n_gen, seed=7, **kw, **extra)
            t = m.last_timing
            ms = t["decode_ms"] / max(1, t["steps"] - 1)
            if rep > 0:
                best[name] = min(ms, best.get(name, ms))
                every.setdefault(name, []).append(round(ms, 5))
    ref = best.get("parent_plain", best["plain"])
    print(f"B={B:3d} n={args.n_gen}: " + ", ".join(f"{k} {v:.4f} ms/token ({(v / ref - 1) * 100:+.2f} %)" for k, v in best.items())
          + f"  [vs {'the parent commit' if args.parent else 'this build'}'s no-filter call]", flush=True)
    report.append(dict(rows=B, n_gen=args.n_gen, rounds=args.rounds, best_ms_per_token=best, all_ms_per_token=every,
                       reference="parent_plain" if args.parent else "plain"))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(dict(filters=FILTERS, odd_rows=OTHER, sampling=kw, precision="bf16", results=report), f, indent=1)
