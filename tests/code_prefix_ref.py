"""CPU restatement of the two code-prefix rules on `oracle.gpt_oracle` -- no engine code.

Resume rule (`generate(code_prefix=)`): a row with prefix p[0 .. k) is the row that had generated those codes itself.  The decode step embeds
code j at mel position j + 2 (kv_cache: the "k + 1 quirk", oracle.gpt_oracle.InferenceModel.forward), so `ResumeModel` prefills
[start, p_0 .. p_{k-1}] at positions [0, 2, 3, .., k + 1]; everything else -- stack, head, processors, draw -- is the oracle's.  In exact
arithmetic its continuation of a run's own prefix is that run's tail.
Reference rule (`inference_speech(input_tokens=)`): the UNCHANGED oracle on cat(fake ids, prefix): positions 0 .. k, then a jump to k + 2.

`continue_run` runs either, `decision_margin` reads a run's smallest decision margin off its trace: the top-2 gap of the processed scores for
greedy, the uniform's distance to the ends of the picked token's CDF interval for sampling (in units of the uniform)."""
import dataclasses
import os

import numpy as np
import torch

from oracle import gpt_oracle as G

MAX_NEW = 40
SETS = [
    dict(do_sample=False, repetition_penalty=1.0),
    dict(do_sample=False, repetition_penalty=10.0),
    dict(do_sample=True, temperature=0.8, top_k=30, top_p=0.8, repetition_penalty=10.0),
    dict(do_sample=True, temperature=1.3, top_k=5, top_p=1.0, repetition_penalty=1.0, typical_mass=0.9),
]
# every compared case must decide with at least this margin: 100 x the largest engine-vs-f64 difference tests/test_gpu_token_scores.py records
MIN_MARGIN = 100 * 1.6809e-6


class ResumeModel(G.InferenceModel):
    """`InferenceModel` (kv_cache=True) whose multi-token prefill puts the codes after the start token at the positions the decode step gives
    them: [0, 2, 3, .., k + 1]"""

    def forward(self, input_ids, attention_mask, past):
        mel_len = self.cached_mel_emb.shape[1]
        if past is not None or input_ids.shape[1] - mel_len <= 1:
            return super().forward(input_ids, attention_mask, past)
        sd, cfg = self.sd, self.cfg
        ids = input_ids[:, mel_len:]
        pos = torch.tensor([0] + list(range(2, ids.shape[1] + 1)))
        e = sd["mel_embedding.weight"][ids] + sd["mel_pos_embedding.emb.weight"][pos]
        pre = self.cached_mel_emb
        if pre.shape[0] != e.shape[0]:
            pre = pre.repeat_interleave(e.shape[0] // pre.shape[0], 0)
        hidden, kv = G.gpt2_stack(sd, cfg, torch.cat([pre, e], dim=1), attention_mask, None)
        return G.lm_head(sd, cfg, hidden), kv


def gen_params(s: dict, max_new: int = MAX_NEW) -> G.GenParams:
    return G.GenParams(do_sample=s["do_sample"], num_beams=1, top_p=s.get("top_p", 1.0), top_k=s.get("top_k", 50),
                       temperature=s.get("temperature", 1.0), repetition_penalty=s["repetition_penalty"],
                       typical_sampling=bool(s.get("typical_mass")), typical_mass=s.get("typical_mass", 0.9), max_generate_length=max_new)


def continue_run(fx, s: dict, prefix: torch.Tensor, rule: str, trace=None) -> torch.Tensor:
    """-> the NEW ids (B, n) after `prefix` (B, k) under settings `s`: rule "resume" (ResumeModel) or "reference" (the unchanged oracle);
    MAX_NEW - k new tokens at most, the uniforms of the rows' own steps k .. (trace: the oracle's per-step logits / scores of the new steps)"""
    sd, cfg = fx["sd"], fx["cfg"]
    k = int(prefix.shape[1])
    with torch.no_grad():
        fake, embeds, mask = G.prepare_gpt_inputs(sd, cfg, G.conds_latent_campplus(sd, fx["style"], fx["emo"]), fx["text"], fx["langs"])
        model = (ResumeModel if rule == "resume" else G.InferenceModel)(sd, cfg, kv_cache=True)
        model.store_mel_emb(embeds)
        inputs = torch.cat([fake, prefix.to(fake.dtype)], dim=1)
        mask = torch.cat([mask, mask.new_ones(mask.shape[0], k)], dim=1)
        out = G.generate_sample(model, inputs, mask, gen_params(s, MAX_NEW - k), fx["uniforms"][k:], trace)
    return out[:, fake.shape[1] + k:]


def decision_margin(trace: dict, new_ids: torch.Tensor, s: dict, uniforms: torch.Tensor, stop: int) -> float:
    """the smallest decision margin over every row's own steps (up to and including its first stop token); uniforms[t, b] is the draw of
    trace step t"""
    worst = float("inf")
    for b in range(new_ids.shape[0]):
        for t in range(new_ids.shape[1]):
            tok = int(new_ids[b, t])
            sc = trace["scores"][t][b]
            if s["do_sample"]:
                p = torch.softmax(sc, dim=-1).double()
                c = p.cumsum(0)
                u = float(uniforms[t, b]) * float(c[-1])
                m = min(u - float(c[tok] - p[tok]), float(c[tok]) - u) / float(c[-1])
            else:
                top = sc.double().topk(2).values
                m = float(top[0] - top[1])
            worst = min(worst, m)
            if tok == stop:
                break
    return worst


_FX = {}


def fixture(golden_dir) -> dict:
    """the tiny model of tests/golden/gpt_greedy.npz as tests/test_gpu_token_scores.py sets it up (4 rows of the longest-running text, the
    fixture's own EOS bias, MAX_NEW = 40, uniforms of seed 7) and the oracle's plain run of every set with its trace; computed once"""
    if _FX:
        return _FX
    z = np.load(os.path.join(golden_dir, "gpt_greedy.npz"))
    c = z["cfg"]
    cfg = G.GPTConfig(layers=int(c[0]), model_dim=int(c[1]), heads=int(c[2]), max_text_tokens=int(c[3]), max_mel_tokens=int(c[4]),
                      number_text_tokens=int(c[5]))
    ref_codes = z["codes"]
    stop_id = int(ref_codes.max())
    ref_lens = [int((r == stop_id).argmax()) if (r == stop_id).any() else r.shape[0] for r in ref_codes]
    long_row = int(np.argmax(ref_lens))
    sd = G.synth_weights(cfg, seed=int(z["seed"]))
    sd["mel_head.bias"][cfg.stop_mel_token] += float(z["eos_bias"])
    fx = dict(cfg=cfg, sd=sd, style=torch.from_numpy(z["style"]), emo=torch.from_numpy(z["emo_vec"]),
              text=torch.from_numpy(z["text"])[long_row:long_row + 1].repeat(4, 1).contiguous(),
              langs=torch.from_numpy(z["langs"])[long_row:long_row + 1].repeat(4).contiguous(),
              uniforms=torch.rand(MAX_NEW, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(7)), stop=cfg.stop_mel_token)
    plain, traces = [], []
    for s in SETS:
        tr = {}
        with torch.no_grad():
            plain.append(G.inference_speech(sd, cfg, G.conds_latent_campplus(sd, fx["style"], fx["emo"]), fx["text"], fx["langs"], gen_params(s),
                                            uniforms=fx["uniforms"], kv_cache=True, trace=tr))
        traces.append(tr)
    fx.update(plain=plain, traces=traces)
    _FX.update(fx)
    return _FX


def n_codes(row: torch.Tensor, stop: int) -> int:
    """codes of a row before its first stop token"""
    hit = (row == stop).nonzero()
    return int(hit[0]) if hit.numel() else int(row.numel())
