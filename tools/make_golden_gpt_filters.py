#!/usr/bin/env python3
"""Mint the logits-filter fixtures tests/golden/gpt_filters_*.npz by running the REFERENCE's own generate() (build container only).

The reference forwards **hf_generate_kwargs into its vendored `GenerationMixin.generate` (indextts/gpt/model_v2.py:815-820), whose
`_get_logits_processor` (indextts/gpt/transformers_generation_utils.py:843-1070) builds the installed transformers.generation.logits_process
classes from them.  Everything that runs the reference comes from tools/make_golden_gpt.py (`build_reference`, `UniformMultinomial`,
`ragged_text`), read from the reference tree at run time; nothing of it is copied here.

Every fixture holds the inputs, the uniform stream, the kwargs (a JSON string), the reference's `codes` and `codes_plain` -- the same call
without the new kwargs.  The tool ASSERTS codes != codes_plain (no fixture is vacuous) and, for sampled cases, that no draw sits within
1e-4 of a CDF edge (a fixture must not rest on a borderline draw); a case that fails either tries its next seed.

usage: make_golden_gpt_filters.py [substring of a case tag]
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_golden_gpt import build_reference, UniformMultinomial, ragged_text, GOLD  # noqa: E402
from oracle import gpt_oracle as G  # noqa: E402

MAX_GEN = 28
MIN_MARGIN = 1e-4


class MarginMultinomial(UniformMultinomial):
    """`UniformMultinomial` that also records the smallest distance of u * total to a CDF edge over every draw it serves."""

    def __init__(self, uniforms):
        super().__init__(uniforms)
        self.margin = float("inf")

    def _note(self, p, u):
        c = p.double().cumsum(0)
        self.margin = min(self.margin, float((c - u * c[-1]).abs().min()))

    def __call__(self, probs, num_samples=1, replacement=False, **kw):
        for b in range(probs.shape[0]):
            us = self.u[self.step, b].reshape(-1)
            p = probs[b].double().clone()
            for j in range(num_samples):
                self._note(p, float(us[j]))
                if num_samples > 1:
                    p[G.inverse_cdf_pick(p, float(us[j]))] = 0.0
        return super().__call__(probs, num_samples, replacement, **kw)


GREEDY = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)
SAMPLE = dict(do_sample=True, num_beams=1, top_p=0.95, top_k=30, temperature=1.0, repetition_penalty=10.0)
SMALL = dict(layers=2, model_dim=128, heads=2)

# tag: (cfg kwargs, seed, B, L, lens, base generate kwargs, filter kwargs, eos_bias, bias on mel id 1)
#   filter values may be callables of (S, codes_plain, cfg): the fake-ids length and the plain run's ids are known only at mint time
CASES = {
    # the shapes, seed and weights of gpt_greedy.npz: codes_plain are that fixture's codes (the sticky-state test runs them on one engine)
    # (when min_new_tokens is given the reference's generate() overwrites min_length with prompt + min_new_tokens, "`min_new_tokens` will take
    # precedence", transformers_generation_utils.py:1445-1453: in `minnew` the larger min_length must NOT hold the stop token back)
    "minnew": (dict(layers=3, model_dim=128, heads=2), 21, 3, 10, [10, 7, 4], GREEDY,
               dict(min_new_tokens=10, min_length=lambda S, c, cfg: S + 15), 2.2, 0.0),
    "minnew4": (dict(layers=3, model_dim=128, heads=2), 21, 3, 10, [10, 7, 4], GREEDY, dict(min_new_tokens=4), 2.2, 0.0),
    "minlen": (dict(layers=3, model_dim=128, heads=2), 21, 3, 10, [10, 7, 4], GREEDY, dict(min_length=lambda S, c, cfg: S + 15), 2.2, 0.0),
    # n = 2 with a bias towards id 1: having emitted 1, the fake prefix [1, ..., 1, start_mel] bans both 1 and start_mel
    "ngram2": (SMALL, 51, 3, 9, [9, 5, 7], dict(GREEDY, repetition_penalty=1.0), dict(no_repeat_ngram_size=2), -1.0, 6.0),
    "ngram3": (SMALL, 52, 3, 9, [9, 6, 8], dict(GREEDY, repetition_penalty=1.0), dict(no_repeat_ngram_size=3), -1.0, 6.0),
    "suppress": (SMALL, 53, 3, 9, [9, 4, 7], GREEDY,
                 dict(suppress_tokens=lambda S, c, cfg: [int(c[0, 2])],
                      begin_suppress_tokens=lambda S, c, cfg: [int(c[1, 0])],
                      bad_words_ids=lambda S, c, cfg: [[int(c[2, 1])], [cfg.stop_mel_token]]), 1.0, 0.0),
    "decay": (SMALL, 54, 3, 9, [9, 6, 8], GREEDY, dict(exponential_decay_length_penalty=(3, 1.25)), -1.0, 0.0),
    "sample_minp": (SMALL, 55, 3, 9, [9, 6, 8], SAMPLE, dict(min_p=0.3), 1.0, 0.0),
    "sample_epsilon": (SMALL, 56, 3, 9, [9, 6, 8], SAMPLE, dict(epsilon_cutoff=0.04), 1.0, 0.0),
    "sample_eta": (SMALL, 57, 3, 9, [9, 6, 8], SAMPLE, dict(eta_cutoff=0.3), 1.0, 0.0),
    "sample_order": (SMALL, 58, 3, 9, [9, 5, 7], dict(SAMPLE, repetition_penalty=1.0),
                     dict(no_repeat_ngram_size=2, min_new_tokens=12, min_p=0.2), 1.5, 2.0),
    "beam_sample": (SMALL, 59, 2, 9, [9, 6], dict(do_sample=True, num_beams=3, top_p=0.95, top_k=8, temperature=1.0, repetition_penalty=10.0,
                                                   length_penalty=0.0),
                    dict(min_new_tokens=8, min_p=0.2, exponential_decay_length_penalty=(9, 1.2)), 1.5, 0.0),
    "beam_suppress": (SMALL, 60, 2, 9, [9, 6], dict(do_sample=False, num_beams=3, repetition_penalty=10.0, length_penalty=0.0),
                      dict(suppress_tokens=lambda S, c, cfg: [int(c[0, 1]), int(c[1, 2])]), 1.2, 0.0),
}


def run(cfg, sd, seed, B, L, lens, gk, fk):
    """one reference call -> (codes, margin, S, inputs)"""
    g = torch.Generator().manual_seed(seed + 100)
    text = ragged_text(g, B, L, cfg.number_text_tokens, lens)
    style = torch.randn(1, 192, generator=g)
    emo_vec = torch.randn(1, cfg.model_dim, generator=g) * 0.1
    langs = torch.randint(0, cfg.n_langs, (B,), generator=g)
    nb = gk.get("num_beams", 1)
    uniforms = torch.rand(MAX_GEN + 2, B, 2 * nb if nb > 1 else 1, generator=g, dtype=torch.float64)
    uv = build_reference(sd, cfg, kv_cache=True)
    seen = {}
    inner = uv.inference_model.generate

    def spy(inputs, *a, **k):
        seen["S"] = int(inputs.shape[1])
        return inner(inputs, *a, **k)
    uv.inference_model.generate = spy
    mm = MarginMultinomial(uniforms)
    with torch.no_grad(), mm:
        codes, _ = uv.inference_speech(torch.zeros(1, 4, 2), text, langs=langs, emo_vec=emo_vec, campplus_embedding=style,
                                       max_generate_length=MAX_GEN, **gk, **fk)
    return codes, mm.margin, seen["S"], dict(text=text, style=style, emo_vec=emo_vec, langs=langs, uniforms=uniforms)


def mint(tag, ck, seed0, B, L, lens, gk, fk_spec, eos_bias, one_bias):
    for seed in range(seed0, seed0 + 4000, 100):          # the next seed when a case does not bite or rests on a borderline draw
        cfg = G.GPTConfig(max_text_tokens=40, max_mel_tokens=60, number_text_tokens=200, **ck)
        sd = G.synth_weights(cfg, seed=seed)
        sd["mel_head.bias"][cfg.stop_mel_token] += eos_bias
        sd["mel_head.bias"][1] += one_bias
        plain, m0, S, inp = run(cfg, sd, seed, B, L, lens, gk, {})
        fk = {k: (v(S, plain, cfg) if callable(v) else v) for k, v in fk_spec.items()}
        codes, m1, _, _ = run(cfg, sd, seed, B, L, lens, gk, fk)
        differs = codes.shape != plain.shape or not bool((codes == plain).all())
        margin = m1                                        # of the run whose ids the engine is held to
        stop = cfg.stop_mel_token
        eos_at = [(int((r == stop).nonzero()[0]) if (r == stop).any() else -1) for r in codes]
        eos_plain = [(int((r == stop).nonzero()[0]) if (r == stop).any() else -1) for r in plain]
        print(f"{tag}: seed {seed} S={S} kwargs={fk} codes {tuple(codes.shape)} eos_at={eos_at} plain {tuple(plain.shape)} eos_at={eos_plain} "
              f"differs={differs} min draw margin={margin:.2e}", flush=True)
        if not differs or (gk.get("do_sample") and margin < MIN_MARGIN):
            continue
        assert differs, "a fixture whose kwargs change nothing checks nothing"
        nb = gk.get("num_beams", 1)
        np.savez_compressed(
            os.path.join(GOLD, f"gpt_filters_{tag}.npz"), text=inp["text"].numpy(), style=inp["style"].numpy(), emo_vec=inp["emo_vec"].numpy(),
            langs=inp["langs"].numpy(), uniforms=inp["uniforms"].numpy(), codes=codes.numpy(), codes_plain=plain.numpy(),
            kwargs=np.array(json.dumps(fk)), seed=np.int64(seed), eos_bias=np.float64(eos_bias), one_bias=np.float64(one_bias),
            kv_cache=np.bool_(True), max_gen=np.int64(MAX_GEN), prompt_len=np.int64(S), margin=np.float64(margin),
            cfg=np.array([cfg.layers, cfg.model_dim, cfg.heads, cfg.max_text_tokens, cfg.max_mel_tokens, cfg.number_text_tokens]),
            gen=np.array([int(gk.get("do_sample", False)), nb, gk.get("top_p", 1.0), gk.get("top_k", 0), gk.get("temperature", 1.0),
                          gk.get("repetition_penalty", 1.0), gk.get("length_penalty", 1.0)], dtype=np.float64))
        return
    raise SystemExit(f"{tag}: no seed makes the kwargs bite with a clear draw margin")


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None
    for tag, spec in CASES.items():
        if only and only not in tag:
            continue
        mint(tag, *spec)


if __name__ == "__main__":
    main()
