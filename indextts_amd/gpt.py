"""Host-side mirror of the reference `UnifiedVoice` decode interface, backed by the HIP engine.

Reference interface mirrored (indextts/gpt/model_v2.py): `UnifiedVoice(**cfg.gpt, spk_cond_mode="campplus")`,
`.load_state_dict`, `.post_init_gpt2_config(kv_cache=, half=)`, `.prepare_gpt_inputs(conds, text, langs)` (:648-714),
`.inference_speech(...)` (:716-825) returning `(codes[:, trunc_index:], speech_conditioning_latent)`, and the
teacher-forced `.forward(...)` latent pass (:596-646).  Input assembly (embedding gathers, left padding) is torch
plumbing on the device; the transformer stack, KV cache, logits processors, token selection and the per-token loop run
inside `libindextts_hip.so` (`itts_gpt_generate`), one hipGraph replay per token.

Prompt encoders (Conformer/Perceiver emotion encoder, CAMPPlus) are out of this path: pass
`emo_vec=` / `campplus_embedding=` computed by the PyTorch-ROCm modules, as `indextts/infer_v2_5.py:762-781` does.
"""
import contextlib
import ctypes as C
import functools
from typing import List, Dict, Optional, Sequence

import torch
import torch.nn.functional as F

from . import _lib


# HF `generate` options that change the generated ids and that the device loop does not implement (the reference forwards every
# hf_generate_kwarg to `GenerationMixin.generate`, model_v2.py:815-820): passing one raises instead of being ignored.
_UNSUPPORTED_GENERATE_KWARGS = frozenset((
    "encoder_no_repeat_ngram_size", "num_beam_groups",
    "diversity_penalty", "penalty_alpha", "early_stopping", "stopping_criteria", "prefix_allowed_tokens_fn", "constraints",
    "force_words_ids", "forced_bos_token_id", "forced_eos_token_id",
    "encoder_repetition_penalty", "renormalize_logits",
    "guidance_scale", "sequence_bias", "typical_p", "assistant_model", "negative_prompt_ids"))

# HF `generate` options the selection kernels apply on the device (itts_gpt_set_logits_filters): the processors and warpers that
# `_get_logits_processor` builds from them (transformers_generation_utils.py:843-1070).  Call-wide as kwargs; per row / beam group as the keys of
# `row_filters` / `group_filters` entries (`row_filter_entries`, itts_gpt_set_row_filters) -- never keys of row_sampling / group_sampling.
_LOGITS_FILTER_KWARGS = ("no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens", "suppress_tokens", "begin_suppress_tokens",
                         "epsilon_cutoff", "eta_cutoff", "exponential_decay_length_penalty", "min_p")
_SUPPORTED_GENERATE_KWARGS = ("do_sample, num_beams, top_p, top_k, temperature, repetition_penalty, length_penalty, typical sampling, "
                              + ", ".join(_LOGITS_FILTER_KWARGS))


def logits_filters(kwargs: dict, vocab: int, stop_token: int, max_new_tokens: int, num_beams: int = 1, who: str = "generate",
                   prompt_len: Optional[int] = None):
    """The one builder behind every decode entry: the `_LOGITS_FILTER_KWARGS` among a generate call's kwargs -> the `_lib.LogitsFilters`
    record the engine installs (itts_gpt_set_logits_filters), or None when HF would build no processor from them.  HF's activation rules
    (transformers_generation_utils.py:843-1070): no_repeat_ngram_size / min_length / min_new_tokens only when > 0, min_p whenever not None,
    epsilon_cutoff / eta_cutoff only strictly inside (0, 1), the rest whenever not None.  Invalid values raise ValueError with the message of
    the transformers.generation.logits_process constructor that rejects them; multi-token bad_words_ids and no_repeat_ngram_size with
    num_beams > 1 raise NotImplementedError.  As in the reference's generate(), a given `min_new_tokens` takes precedence over `min_length`
    (it overwrites it with prompt + min_new_tokens, :1445-1453), and with `prompt_len` (the fake-ids length S) known, a minimum beyond
    prompt_len + max_new_tokens is the "Unfeasible length constraints" ValueError of :1398-1410."""
    g = lambda k: kwargs.get(k)
    f = _lib.LogitsFilters()
    f.min_p = -1.0
    on = False

    def count(name, label):                     # MinLength / MinNewTokensLength / NoRepeatNGram: an int, active when > 0
        v = g(name)
        if v is None or isinstance(v, bool) or not v > 0:
            return 0
        if not isinstance(v, int):
            raise ValueError(label.format(v))
        return int(v)

    def ids_of(name, seq):
        out = []
        for t in seq:
            if isinstance(t, bool) or not isinstance(t, int) and not (hasattr(t, "__index__")):
                raise ValueError(f"{who}: `{name}` has to be a list of token ids, but holds {t!r}")
            t = int(t)
            if not 0 <= t < vocab:
                raise ValueError(f"{who}: `{name}` id {t} is outside the vocabulary (0 .. {vocab - 1})")
            out.append(t)
        return out

    f.no_repeat_ngram_size = count("no_repeat_ngram_size", "`ngram_size` has to be a strictly positive integer, but is {}")
    if f.no_repeat_ngram_size and int(num_beams) != 1:
        raise NotImplementedError(f"{who}: no_repeat_ngram_size is implemented for num_beams = 1 only (a beam's n-gram history needs a per-beam "
                                  "sequence buffer reordered with the beams, which the beam kernels do not keep)")
    f.min_new_tokens = count("min_new_tokens", "`min_new_tokens` has to be a positive integer, but is {}")
    f.min_length = 0 if g("min_new_tokens") is not None else count("min_length", "`min_length` has to be a non-negative integer, but is {}")
    if prompt_len is not None:
        max_length = int(prompt_len) + int(max_new_tokens)
        if f.min_length > max_length:
            raise ValueError(f"Unfeasible length constraints: `min_length` ({f.min_length}) is larger than the maximum possible length ({max_length}).")
        if f.min_new_tokens + int(prompt_len) > max_length:
            raise ValueError(f"Unfeasible length constraints: `min_new_tokens` ({f.min_new_tokens}), when added to the prompt length "
                             f"({prompt_len}), is larger than the maximum possible length ({max_length}).")
    on = bool(f.no_repeat_ngram_size or f.min_length or f.min_new_tokens)

    suppress = []
    bad = g("bad_words_ids")
    if bad is not None:                         # NoBadWordsLogitsProcessor._validate_arguments, then its [eos] filter
        if not isinstance(bad, list) or len(bad) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bad}.")
        if any(not isinstance(w, list) for w in bad):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bad}.")
        if any(any(isinstance(t, bool) or not hasattr(t, "__index__") or t < 0 for t in w) for w in bad):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bad}.")
        if any(len(w) == 0 for w in bad):
            raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {bad}.")
        words = [w for w in bad if [int(t) for t in w] != [int(stop_token)]]
        if any(len(w) > 1 for w in words):
            raise NotImplementedError(f"{who}: bad_words_ids with multi-token entries {[w for w in words if len(w) > 1]} is not implemented: "
                                      "the device filter bans single ids (a word of several tokens needs the row's history matched per word)")
        suppress += ids_of("bad_words_ids", [w[0] for w in words])
    if g("suppress_tokens") is not None:
        suppress += ids_of("suppress_tokens", list(g("suppress_tokens")))
    begin = ids_of("begin_suppress_tokens", list(g("begin_suppress_tokens"))) if g("begin_suppress_tokens") is not None else []

    decay = []
    ed = g("exponential_decay_length_penalty")
    if ed is not None:
        if not isinstance(ed, (tuple, list)) or len(ed) != 2 or isinstance(ed[0], bool) or not isinstance(ed[0], int) or ed[0] < 0 \
                or isinstance(ed[1], bool) or not isinstance(ed[1], (int, float)) or not ed[1] > 0:
            raise ValueError(f"`exponential_decay_length_penalty` has to be a (start_index >= 0, decay_factor > 0) tuple, but is {ed}")
        start, factor = int(ed[0]), ed[1]

        def mult(t):                            # HF: pow(regulation_factor, penalty_idx) - 1 as a Python float, multiplied into an f32 tensor
            try:
                return float(pow(factor, t - start) - 1)
            except OverflowError:
                return float("inf")
        decay = [mult(t) if t > start else 0.0 for t in range(int(max_new_tokens))]
        f.decay_start = start

    if g("min_p") is not None:
        mp = g("min_p")
        if not (0 <= mp <= 1.0):
            raise ValueError(f"`min_p` has to be a float in the [0, 1] interval, but is {mp}")
        f.min_p = float(mp)
        on = True
    for name in ("epsilon_cutoff", "eta_cutoff"):
        v = g(name)
        if v is not None and 0.0 < v < 1.0:
            setattr(f, name, float(v))
            on = True
    if not (on or suppress or begin or decay):
        return None
    arr = lambda typ, vals: (typ * len(vals))(*vals) if vals else None
    keep = (arr(C.c_int32, suppress), arr(C.c_int32, begin), arr(C.c_float, decay))
    f.n_suppress, f.n_begin_suppress, f.n_decay = len(suppress), len(begin), len(decay)
    if keep[0] is not None:
        f.suppress_ids = keep[0]
    if keep[1] is not None:
        f.begin_suppress_ids = keep[1]
    if keep[2] is not None:
        f.decay_table = keep[2]
    f._keep = keep                              # the record points into these
    return f


def off_filters():
    """The "off" record of a per-slot filter table: a row without filters (all counts 0, no decay, min_p off, cutoffs 0, no ids) -- under it
    the selection kernels compute the bits of the unfiltered path."""
    f = _lib.LogitsFilters()
    f.min_p = -1.0
    return f


class _FilterTable(list):
    """the `_lib.LogitsFilters` records of a per-slot filter table (`row_filter_entries`), as `_install_filters` takes them"""


def row_filter_entries(rows, n: int, call_kwargs: dict, vocab: int, stop_token: int, max_new_tokens: int, num_beams: int = 1,
                       who: str = "generate", prompt_len: Optional[int] = None, row_max_new: Optional[Sequence[int]] = None,
                       name: str = "row_filters") -> list:
    """`row_filters=` (num_beams = 1) / `group_filters=` (beam groups) of the decode entries -> `n` `_lib.LogitsFilters` records, the engine's
    per-slot filter table (itts_gpt_set_row_filters).  rows: one entry per row -- a dict of `_LOGITS_FILTER_KWARGS` keys, or None (= {}).  The
    entry is merged over the call's own filter kwargs (`call_kwargs`; other keys are ignored): a key the entry HAS wins, whatever its value
    (None is HF's default: that filter is off for the row), a key it lacks takes the call's value.  The merged kwargs of every row go
    through `logits_filters`, so HF's rules hold per row: its validation and messages (prefixed with the entry), `min_new_tokens` over
    `min_length`, the feasibility check against the row's own cap (min(max_new_tokens, row_max_new[i])) and `prompt_len`, and the
    refusals (multi-token bad words; no_repeat_ngram_size with num_beams > 1).  A row whose merged kwargs build nothing gets `off_filters()`.
    Unknown keys raise ValueError."""
    rows = list(rows)
    if len(rows) != n:
        raise ValueError(f"{name} must have one entry per {'row' if int(num_beams) == 1 else 'utterance'} ({n}), got {len(rows)}")
    if row_max_new is not None and len(row_max_new) != n:
        raise ValueError(f"row_max_new must have one entry per row ({n}), got {len(row_max_new)}")
    base = {k: call_kwargs[k] for k in _LOGITS_FILTER_KWARGS if k in call_kwargs}
    out = []
    for i, r in enumerate(rows):
        r = {} if r is None else r
        if not isinstance(r, dict):
            raise TypeError(f"{name}[{i}] must be a dict or None, got {type(r).__name__}")
        unknown = sorted(set(r) - set(_LOGITS_FILTER_KWARGS))
        if unknown:
            raise ValueError(f"{name}[{i}]: unknown keys {unknown} (known: {list(_LOGITS_FILTER_KWARGS)})")
        merged = dict(base, **r)
        cap = int(max_new_tokens) if row_max_new is None else min(int(max_new_tokens), int(row_max_new[i]))
        try:
            if cap != int(max_new_tokens):      # the row's own feasibility; its decay table still spans the call's steps, as decoded alone
                logits_filters(merged, vocab, stop_token, cap, num_beams, who, prompt_len)
            f = logits_filters(merged, vocab, stop_token, int(max_new_tokens), num_beams, who, prompt_len)
        except (ValueError, NotImplementedError) as e:
            raise type(e)(f"{name}[{i}]: {e}") from e
        out.append(off_filters() if f is None else f)
    return out


def _reject_logits_processor(hf_generate_kwargs: dict):
    """The reference builds its own `logits_processor` list and passes it beside **hf_generate_kwargs (model_v2.py:793-799,815-820;
    model.py:655-660), so a caller-supplied one is a TypeError there (duplicate keyword); the same error here, not a silent drop."""
    if "logits_processor" in hf_generate_kwargs:
        raise TypeError("inference_speech() got multiple values for keyword argument 'logits_processor' (the reference passes its own "
                        "LogitsProcessorList to generate; use typical_sampling / typical_mass)")


_ROW_SAMPLING_KEYS = ("do_sample", "top_k", "top_p", "temperature", "repetition_penalty", "typical_mass", "min_tokens_to_keep", "stream", "seed")
_GROUP_SAMPLING_KEYS = _ROW_SAMPLING_KEYS + ("length_penalty",)


def _sampling_entries(name: str, per: str, record, keys, default_keep: int, rows, n: int, defaults: dict, slots) -> list:
    """The validator behind `row_sampling_entries` / `group_sampling_entries`: `n` `record`s (`_lib.RowSampling` / `_lib.GroupSampling`) from
    one dict per `per` (row / utterance).  name: the table's name in the messages; keys: the known keys (`length_penalty` among them: the
    record has that field); default_keep: min_tokens_to_keep where neither the entry nor `defaults` has one."""
    rows = list(rows)
    if len(rows) != n:
        raise ValueError(f"{name} must have one entry per {per} ({n}), got {len(rows)}")
    out = []
    for i, r in enumerate(rows):
        if not isinstance(r, dict):
            raise TypeError(f"{name}[{i}] must be a dict, got {type(r).__name__}")
        unknown = sorted(set(r) - set(keys))
        if unknown:
            raise ValueError(f"{name}[{i}]: unknown keys {unknown} (known: {list(keys)})")
        g = lambda k: r[k] if r.get(k) is not None else defaults[k]
        e = record()
        e.do_sample, e.top_k = int(bool(g("do_sample"))), int(g("top_k") or 0)
        e.min_tokens_to_keep = int(r["min_tokens_to_keep"] if r.get("min_tokens_to_keep") is not None else defaults.get("min_tokens_to_keep", default_keep))
        e.top_p, e.temperature, e.repetition_penalty = float(g("top_p")), float(g("temperature")), float(g("repetition_penalty"))
        e.typical_mass = float(g("typical_mass") or 0.0)
        if "length_penalty" in keys:
            e.length_penalty = float(g("length_penalty"))
        stream = int(r["stream"]) if r.get("stream") is not None else int(slots[i] if slots is not None else i)
        if not -2 ** 31 <= stream < 2 ** 31:
            raise ValueError(f"{name}[{i}]: stream must fit an int32 (got {stream})")
        e.stream = stream
        e.seed = int(g("seed")) & 0xFFFFFFFFFFFFFFFF
        if e.do_sample and not 1 <= e.top_k <= 64:
            raise ValueError(f"{name}[{i}]: top_k must be in 1..64 on the device path (got {e.top_k})")
        if e.typical_mass != 0.0 and not 0.0 < e.typical_mass < 1.0:
            raise ValueError(f"{name}[{i}]: `typical_mass` has to be a float > 0 and < 1, but is {e.typical_mass}")
        if not e.repetition_penalty > 0.0 or not e.temperature > 0.0:
            raise ValueError(f"{name}[{i}]: repetition_penalty ({e.repetition_penalty}) and temperature ({e.temperature}) must be > 0")
        if not 0 <= e.min_tokens_to_keep <= 2:
            raise ValueError(f"{name}[{i}]: min_tokens_to_keep must be in 0..2 (got {e.min_tokens_to_keep})")
        out.append(e)
    return out


def row_sampling_entries(rows, n: int, defaults: dict, slots: Optional[Sequence[int]] = None) -> list:
    """`row_sampling=` of `generate` / `DecodeSession` -> `n` `_lib.RowSampling` records (the engine's per-slot sampling table,
    itts_gpt_set_row_sampling).  rows: one dict per row; a missing key takes the call's scalar from `defaults`, a missing `stream` the slot
    index (`slots[i]`, default i) -- so the same entry in every row reproduces the scalar call.  Raises for what the engine rejects: unknown
    keys, do_sample with top_k outside 1..64, typical_mass outside (0, 1) unless 0, repetition_penalty / temperature <= 0."""
    return _sampling_entries("row_sampling", "row", _lib.RowSampling, _ROW_SAMPLING_KEYS, 1, rows, n, defaults, slots)


def group_sampling_entries(rows, n: int, defaults: dict, slots: Optional[Sequence[int]] = None) -> list:
    """`group_sampling=` of `generate(num_beams > 1)` / `BeamDecodeSession` -> `n` `_lib.GroupSampling` records (the beam kernels' per-group
    sampling table, itts_gpt_set_group_sampling): `row_sampling_entries` for beam groups, with `length_penalty` as one more key.  rows: one dict
    per utterance; a missing key takes the call's scalar from `defaults`, a missing `stream` the slot index (`slots[i]`, default i) -- so the
    same entry in every group reproduces the scalar call.  min_tokens_to_keep defaults to 2: one eos id -> the beam warpers keep eos + 1
    (generation_utils.py:1023-1029).  Raises for what the engine rejects: unknown keys, do_sample with top_k outside 1..64, typical_mass
    outside (0, 1) unless 0, repetition_penalty / temperature <= 0, min_tokens_to_keep outside 0..2."""
    return _sampling_entries("group_sampling", "utterance", _lib.GroupSampling, _GROUP_SAMPLING_KEYS, 2, rows, n, defaults, slots)


def _sampling_bytes(entries) -> torch.Tensor:
    """host image (n, record size) uint8 of a list of `_lib.RowSampling` (40 bytes) or `_lib.GroupSampling` (48 bytes) records"""
    record = type(entries[0])
    arr = (record * len(entries))(*entries)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).view(len(entries), C.sizeof(record))


_row_sampling_bytes = _group_sampling_bytes = _sampling_bytes


def _gp_defaults(gp) -> dict:
    """the call's scalar sampling settings, as the defaults of its `row_sampling` entries"""
    return dict(do_sample=gp.do_sample, top_k=gp.top_k, top_p=gp.top_p, temperature=gp.temperature, repetition_penalty=gp.repetition_penalty,
                typical_mass=gp.typical_mass, seed=gp.seed)


def _gp_group_defaults(gp) -> dict:
    """the beam call's scalar settings, as the defaults of its `group_sampling` entries"""
    return dict(_gp_defaults(gp), length_penalty=gp.length_penalty, min_tokens_to_keep=gp.min_tokens_to_keep)


def _gen_params(kv_cache: bool, max_new_tokens: int, seed: int, do_sample=False, num_beams=1, top_p=1.0, top_k=50, temperature=1.0,
                repetition_penalty=1.0, length_penalty=1.0, typical_mass=0.0):
    """The engine's `GenParams` of a generate call / session; seed: the resolved device seed (`UnifiedVoice._seed`).  Beam calls keep two
    tokens: one eos id -> the warpers keep eos + 1 (generation_utils.py:1023-1029)."""
    gp = _lib.GenParams()
    gp.do_sample, gp.num_beams, gp.top_k = int(bool(do_sample)), int(num_beams), int(top_k or 0)
    gp.min_tokens_to_keep, gp.max_new_tokens = 1 if int(num_beams) == 1 else 2, int(max_new_tokens)
    gp.pos_offset = 2 if kv_cache else 1
    gp.top_p, gp.temperature = float(top_p), float(temperature)
    gp.repetition_penalty = float(repetition_penalty if repetition_penalty is not None else 1.0)
    gp.length_penalty, gp.seed = float(length_penalty), int(seed)
    gp.typical_mass = float(typical_mass)
    return gp


def _any_group_samples(do_sample, group_sampling) -> bool:
    """does the call draw random numbers: its scalar do_sample, or any entry's own"""
    return bool(do_sample) or any(isinstance(r, dict) and bool(r.get("do_sample")) for r in (group_sampling or ()))


def beam_steps_run(hyps, n_hyps, done, steps: int) -> int:
    """The step count the reference's beam loop ends at: the first step after which every utterance is done (the engine checks its flags
    every few steps and may idle past it), else `steps` (max_length)."""
    hy_i = hyps.view("int32")
    if len(done) and all(bool(d) for d in done):
        last = max(int(hy_i[b, q, 1]) for b in range(len(done)) for q in range(int(n_hyps[b])))
        return min(int(steps), last + 1)
    return int(steps)


def finalize_beam_group(hist_tok, hist_par, beam_scores, hyps, n_hyps, done, own_steps: int, length_penalty: float, group: int = 0,
                        num_beams: Optional[int] = None) -> List[int]:
    """`BeamSearchScorer.finalize` (transformers_beam_search.py:320-408) for ONE utterance (beam group) on the host: the ids of its best
    hypothesis.  numpy views of the engine's search state: hist_tok / hist_par [steps][rows] (chosen token / parent row per own step),
    beam_scores [rows], hyps [groups][4][4] f32 records {f32 score, i32 step, i32 row, pad}, n_hyps / done [groups].  A group that is not
    done adds its open beams with generated_len = own_steps (the steps its search ran: max_length, or its cap in a session)."""
    b = int(group)
    nb = int(num_beams) if num_beams is not None else len(beam_scores) // len(done)
    hy_i = hyps.view("int32")

    def seq_of(row: int, upto: int):
        toks = []
        r = row
        for sidx in range(upto, -1, -1):
            toks.append(int(hist_tok[sidx, r]))
            r = int(hist_par[sidx, r])
        return toks[::-1]

    heap = [(float(hyps[b, q, 0]), seq_of(int(hy_i[b, q, 2]), int(hy_i[b, q, 1]) - 1) if int(hy_i[b, q, 1]) > 0 else [])
            for q in range(int(n_hyps[b]))]
    if not done[b]:
        worst = min([h0[0] for h0 in heap], default=1e9) if len(heap) >= nb else 1e9
        for j in range(nb):                         # open beams join the heap with generated_len = own_steps
            row = b * nb + j
            sc = float(beam_scores[row]) / (int(own_steps) ** float(length_penalty))
            if len(heap) < nb or sc > worst:
                heap.append((sc, seq_of(row, int(own_steps) - 1)))
                if len(heap) > nb:
                    heap.remove(min(heap, key=lambda t: t[0]))
                worst = min(t[0] for t in heap)
    return sorted(heap, key=lambda t: t[0])[-1][1]


class TokenScores:
    """Per-token log-probabilities of a `generate(..., token_scores=True)` call (itts_gpt_set_token_scores; what `output_scores` plus
    `compute_transition_scores(normalize_logits=True)` give in the vendored generation utils): logp_model (B, n) f32 = log_softmax(raw logits)
    of the stored token, logp_sampled (B, n) f32 = the log-probability it was selected with (after penalty, filters and warpers), lengths (B,)
    = the tokens the MODEL chose in each row (a stop token of its own counts; forced tokens -- past a row's end or cap -- do not and hold
    0.0), ended (B,) bool = the row's stop token was the model's own (False: it ran into its cap).
    `logp_sampled=None`: the record of a rescoring pass (`UnifiedVoice.rescore`), which scores given codes under the model's own distribution
    and has no selection to report: `of="sampled"` then raises.
    `starts` (B,), optional: the columns a row was GIVEN (`generate(code_prefix=)`): they hold 0.0, as forced tokens do, `lengths` counts
    them (the columns line up with the codes) and `mean_logprob` / `min_logprob` skip them.  None: every row starts at column 0."""

    def __init__(self, logp_model: torch.Tensor, logp_sampled: Optional[torch.Tensor], lengths, ended, starts=None):
        self.logp_model, self.logp_sampled = logp_model, logp_sampled
        self.lengths = torch.as_tensor(lengths).to(torch.int64).reshape(-1).cpu()
        self.ended = torch.as_tensor(ended).to(torch.bool).reshape(-1).cpu()
        self.starts = None if starts is None else torch.as_tensor(starts).to(torch.int64).reshape(-1).cpu()
        if not ((logp_sampled is None or logp_model.shape == logp_sampled.shape) and logp_model.dim() == 2 and
                self.lengths.numel() == logp_model.shape[0] == self.ended.numel()):
            raise ValueError("TokenScores: logp_model / logp_sampled (B, n), lengths (B,), ended (B,)")
        if self.starts is not None and (self.starts.numel() != self.lengths.numel() or bool((self.starts < 0).any())):
            raise ValueError("TokenScores: starts (B,) >= 0")

    @staticmethod
    def lengths_of(codes: torch.Tensor, caps: Sequence[int], stop_token: int):
        """(lengths, ended) of code rows (B, W) that hold the stop token from each row's end on: a row whose first stop token sits before its
        cap chose it itself (ended, length = its column + 1); otherwise the row ran into its cap (min(cap, W) tokens of its own)."""
        c = codes.detach().cpu()
        W = int(c.shape[1])
        lengths, ended = [], []
        for b in range(c.shape[0]):
            cap = max(0, min(W, int(caps[b])))
            hit = (c[b] == int(stop_token)).nonzero()
            first = int(hit[0]) if hit.numel() else W
            ended.append(first < cap)
            lengths.append(first + 1 if first < cap else cap)
        return torch.tensor(lengths, dtype=torch.int64), torch.tensor(ended, dtype=torch.bool)

    def _rows(self, of: str):
        if of not in ("model", "sampled"):
            raise ValueError("TokenScores: of must be 'model' or 'sampled'")
        if of == "sampled" and self.logp_sampled is None:
            raise ValueError("TokenScores: a rescoring pass has no logp_sampled (the codes were given, not selected)")
        a = (self.logp_model if of == "model" else self.logp_sampled).detach().to("cpu", torch.float64)
        s0 = [0] * len(self.lengths) if self.starts is None else self.starts.tolist()
        return [a[b, min(int(s), int(n)): int(n)] for b, (s, n) in enumerate(zip(s0, self.lengths.tolist()))]

    def mean_logprob(self, of: str = "model") -> torch.Tensor:
        """(B,) f64: the mean over each row's `lengths` entries (from `starts` on) of logp_model (of="sampled": logp_sampled), on the host;
        nan when there is none"""
        return torch.tensor([float(r.sum() / r.numel()) if r.numel() else float("nan") for r in self._rows(of)], dtype=torch.float64)

    def min_logprob(self, of: str = "model") -> torch.Tensor:
        """(B,) f64: the least of each row's `lengths` entries (from `starts` on); nan when there is none"""
        return torch.tensor([float(r.min()) if r.numel() else float("nan") for r in self._rows(of)], dtype=torch.float64)

    def row(self, b: int) -> "TokenScores":
        return TokenScores(self.logp_model[b:b + 1], None if self.logp_sampled is None else self.logp_sampled[b:b + 1], self.lengths[b:b + 1],
                           self.ended[b:b + 1], None if self.starts is None else self.starts[b:b + 1])

    @staticmethod
    def stack(rows: Sequence["TokenScores"], device=None) -> "TokenScores":
        """one record of single-row records, zero-padded (a forced column holds 0.0) to the widest"""
        W = max(int(r.logp_model.shape[1]) for r in rows)
        pad = lambda t: F.pad(t, (0, W - int(t.shape[1])))
        cat = lambda ts: torch.cat([pad(t if device is None else t.to(device)) for t in ts], 0)
        sampled = None if any(r.logp_sampled is None for r in rows) else cat([r.logp_sampled for r in rows])
        starts = None if all(r.starts is None for r in rows) else torch.cat([torch.zeros_like(r.lengths) if r.starts is None else r.starts for r in rows])
        return TokenScores(cat([r.logp_model for r in rows]), sampled, torch.cat([r.lengths for r in rows]), torch.cat([r.ended for r in rows]), starts)


ALIGN_MAX_PAIRS, ALIGN_MAX_TEXT, ALIGN_MAX_KEYS = 8, 1024, 12288          # itts_gpt_set_alignment's bounds (gpt_kernels.h)


def alignment_pairs(heads, layers: int, n_heads: int, who: str = "generate") -> list:
    """`alignment_heads=[(layer, head), ...]` checked against the model: 1 .. 8 distinct pairs inside layers x heads -> [(layer, head)] of ints"""
    try:
        pairs = [(int(l), int(h)) for l, h in heads]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: alignment_heads must be a sequence of (layer, head) pairs, got {heads!r}") from None
    if not 1 <= len(pairs) <= ALIGN_MAX_PAIRS:
        raise ValueError(f"{who}: alignment_heads takes 1 .. {ALIGN_MAX_PAIRS} (layer, head) pairs, got {len(pairs)}")
    bad = [p for p in pairs if not (0 <= p[0] < layers and 0 <= p[1] < n_heads)]
    if bad:
        raise ValueError(f"{who}: alignment_heads {bad} lie outside the model's {layers} layers x {n_heads} heads")
    if len(set(pairs)) != len(pairs):
        raise ValueError(f"{who}: alignment_heads lists a (layer, head) pair twice: {pairs}")
    return pairs


def alignment_spans(spans, n: int, who: str = "generate") -> list:
    """`text_spans=[(off, len), ...]`: one per utterance, 0 <= off <= 12288 keys after the row's first valid key, 0 <= len <= 1024 -> [(off, len)] of ints"""
    if spans is None:
        raise ValueError(f"{who}: alignment_heads needs text_spans=[(off, len), ...], the text's key span of every utterance (relative to the "
                         "row's first valid key; the inference_speech entries derive it from prepare_gpt_inputs)")
    try:
        out = [(int(o), int(l)) for o, l in spans]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: text_spans must be a sequence of (off, len) pairs, got {spans!r}") from None
    if len(out) != n:
        raise ValueError(f"{who}: text_spans must have one entry per utterance ({n}), got {len(out)}")
    bad = [v for v in out if not 0 <= v[0] <= ALIGN_MAX_KEYS or not 0 <= v[1] <= ALIGN_MAX_TEXT]
    if bad:
        raise ValueError(f"{who}: text_spans {bad}: 0 <= off <= {ALIGN_MAX_KEYS} (no cache row is longer) and 0 <= len <= {ALIGN_MAX_TEXT}")
    return out


def refuse_code_prefix(kwargs: dict, who: str) -> None:
    """the pipelines' entries other than the v2.5 `infer_requests`: `code_prefix` is a REQUEST key there (one sequence per segment); a
    call-wide kwarg would reach `generate` as the prefix of whatever batch the pipeline happens to build"""
    if any(kwargs.get(k) is not None for k in ("code_prefix", "code_prefix_lens", "input_tokens")):
        raise ValueError(f"{who}: code_prefix is a request key of the IndexTTS-2.5 `infer_requests` (one code sequence per segment); "
                         "it is not available here")


def _refuse_timestamps(kwargs: dict, who: str) -> None:
    """`timestamps=True` belongs to `IndexTTS2.infer_requests` (the v2.5 pipeline): anywhere else it would be dropped silently"""
    if kwargs.get("timestamps"):
        raise ValueError(f"{who}: timestamps=True is implemented by IndexTTS2.infer_requests (IndexTTS-2.5, num_beams = 1) only; this entry takes "
                         "alignment_heads= and leaves the text attention in last_alignment")


def _alignment_text_cap(spans) -> int:
    return max(4, (max(l for _, l in spans) + 3) // 4 * 4)


def monotonic_path(logp) -> list:
    """Monotonic alignment search: the path j(0) = 0, j(n - 1) = T - 1, j(i + 1) - j(i) in {0, 1} of the greatest sum of logp[i][j(i)] over
    an (n, T) matrix with n >= T >= 1 (dynamic programme in f64; of two equal predecessors the one that stays wins) -> [j(i)]."""
    import numpy as np
    a = np.asarray(logp, dtype=np.float64)
    n, T = a.shape
    if not 1 <= T <= n:
        raise ValueError(f"monotonic_path: {n} codes cannot cover {T} text positions in steps of 0 / +1")
    Q = np.full((n, T), -np.inf)
    Q[0, 0] = a[0, 0]
    for i in range(1, n):
        stay, move = Q[i - 1], np.concatenate(([-np.inf], Q[i - 1, :-1]))
        Q[i] = a[i] + np.maximum(stay, move)
    path, j = [0] * n, T - 1
    for i in range(n - 1, -1, -1):
        path[i] = j
        if i and j and not Q[i - 1, j] >= Q[i - 1, j - 1]:
            j -= 1
    return path


class TokenAlignment:
    """The text attention of a `generate(..., alignment_heads=[(layer, head), ...], text_spans=...)` call (itts_gpt_set_alignment): attn
    (B, n, K, text_cap) f32 -- row i of utterance b holds, for the K selected pairs, the softmax weights of the query that PREDICTED code i
    over the utterance's text keys (columns 0 .. text_lens[b] - 1; columns from text_lens[b] on are zero here).  Row 0 is zero (code 0 comes
    from the prefill, whose attention is not exported) and so are forced columns (past a row's end or cap).  text_lens (B,): the span
    lengths; lengths (B,): the tokens the model chose in each row, as `TokenScores.lengths`.  The columns are those of the returned ids."""
    EPS = 1e-8

    def __init__(self, attn: torch.Tensor, text_lens, lengths):
        self.attn = attn
        self.text_lens = torch.as_tensor(text_lens).to(torch.int64).reshape(-1).cpu()
        self.lengths = torch.as_tensor(lengths).to(torch.int64).reshape(-1).cpu()
        if not (attn.dim() == 4 and self.text_lens.numel() == attn.shape[0] == self.lengths.numel()):
            raise ValueError("TokenAlignment: attn (B, n, K, text_cap), text_lens (B,), lengths (B,)")

    def row(self, b: int) -> "TokenAlignment":
        return TokenAlignment(self.attn[b:b + 1], self.text_lens[b:b + 1], self.lengths[b:b + 1])

    @staticmethod
    def stack(rows: Sequence["TokenAlignment"], device=None) -> "TokenAlignment":
        """one record of single-row records, zero-padded to the widest in codes and in text"""
        W, Tc = max(int(r.attn.shape[1]) for r in rows), max(int(r.attn.shape[3]) for r in rows)
        pad = lambda t: F.pad(t, (0, Tc - int(t.shape[3]), 0, 0, 0, W - int(t.shape[1])))
        return TokenAlignment(torch.cat([pad(r.attn if device is None else r.attn.to(device)) for r in rows], 0),
                              torch.cat([r.text_lens for r in rows]), torch.cat([r.lengths for r in rows]))

    def _matrix(self, row: int, reduce, n_codes: Optional[int]):
        """(n, T) f64 on the host: the utterance's first n code rows over its text positions, the K pairs reduced"""
        T = int(self.text_lens[row])
        n = int(self.lengths[row]) if n_codes is None else int(n_codes)
        n = max(0, min(n, int(self.attn.shape[1])))
        a = self.attn[row, :n, :, :T].detach().to("cpu", torch.float64)
        if reduce == "mean":
            return a.mean(1)
        if reduce == "max":
            return a.max(1).values
        if isinstance(reduce, int) and not isinstance(reduce, bool) and 0 <= reduce < a.shape[1]:
            return a[:, reduce]
        raise ValueError(f"TokenAlignment: reduce must be 'mean', 'max' or a pair index 0 .. {a.shape[1] - 1}, got {reduce!r}")

    def path(self, row: int, reduce="mean", n_codes: Optional[int] = None) -> torch.Tensor:
        """Monotonic alignment search over log(p + eps) of the head-reduced matrix (`reduce`: "mean" / "max" over the pairs, or one pair's
        index) of utterance `row`'s first n_codes codes (default: `lengths[row]`): code 0 is pinned to text position 0 and the last code to
        the last position, the text index never decreases and moves by 0 or +1 per code.  Returns (T, 2) int64: [start_code, end_code) per
        text position.  Fewer codes than text positions: only the first n_codes positions are aligned (one code each), the others get the
        empty range [n_codes, n_codes)."""
        a = self._matrix(row, reduce, n_codes)
        n, T = int(a.shape[0]), int(a.shape[1])
        out = torch.full((T, 2), n, dtype=torch.int64)
        Ta = min(T, n)
        if Ta < 1:
            return out
        p = monotonic_path(torch.log(a[:, :Ta] + self.EPS).numpy())
        for j in range(Ta):
            idx = [i for i, v in enumerate(p) if v == j]
            out[j, 0], out[j, 1] = idx[0], idx[-1] + 1
        return out

    def monotonicity(self) -> torch.Tensor:
        """(B, K) f64: per utterance and pair, the share of that pair's attention mass (over the utterance's code rows and text positions) that
        lies on the pair's OWN monotonic path -- 1.0 for a one-hot staircase, about 1 / T for a head that ignores the text order; nan where
        there is no mass or fewer codes than text positions.  Ranks heads on a checkpoint."""
        B, K = int(self.attn.shape[0]), int(self.attn.shape[2])
        out = torch.full((B, K), float("nan"), dtype=torch.float64)
        for b in range(B):
            for k in range(K):
                a = self._matrix(b, k, None)
                n, T = int(a.shape[0]), int(a.shape[1])
                tot = float(a.sum())
                if T < 1 or n < T or not tot > 0.0:
                    continue
                p = monotonic_path(torch.log(a + self.EPS).numpy())
                out[b, k] = float(sum(a[i, j] for i, j in enumerate(p))) / tot
        return out


class _HandleState(contextlib.ExitStack):
    """What ONE decode call or session has installed on `model`'s engine handle (the sticky state of the itts_gpt_set_* entries), and the one way
    it leaves again.  Every method registers the clearing call BEFORE it calls the setter: a setter that fails half-way is still cleared, and
    clearing what was never set is a no-op in the engine.  Leaving the `with` block, or `close()`, runs the clearing calls in reverse order,
    each of them even if another raises.  An argument of None installs nothing.  A call holds one around its engine call, a session from the
    first step of its __init__ until close(); a code prefix, which lives for one engine call of a session, gets a nested one."""

    def __init__(self, model: "UnifiedVoice"):
        super().__init__()
        self.m, self._resets_threshold = model, False

    def filters(self, filt) -> None:
        if filt is not None:
            self.callback(self.m._uninstall_filters, filt)
            self.m._install_filters(filt)

    def prefix(self, prefix, prefix_chunk: int, pos_offset: Optional[int]) -> None:
        if prefix is not None:
            self.callback(self.m._uninstall_prefix)
            self.m._install_prefix(prefix, prefix_chunk, pos_offset)

    def sampling(self, kind: str, entries):
        """-> the installed table"""
        if entries is not None:
            self.callback(self.m._uninstall_sampling, kind)
            return self.m._install_sampling(kind, entries)

    def scores(self, on: bool, B: int, max_new: int):
        """-> (logp_model, logp_sampled)"""
        if on:
            self.callback(self.m._uninstall_scores)
            return self.m._install_scores(B, max_new)

    def alignment(self, req, B: int, max_new: int, text_cap: Optional[int] = None):
        """-> (span, out)"""
        if req is not None:
            self.callback(self.m._uninstall_alignment)
            return self.m._install_alignment(req, B, max_new, text_cap)

    def row_limits(self, row_max_new, B: int):
        """per-row token caps -> their buffer (persistent: its address is part of the decode graph's key).  None: the entry is still called,
        with NULL -- which clears"""
        lim, set_limits = None, _lib.lib().itts_gpt_set_row_limits
        if row_max_new is not None:
            if len(row_max_new) != B:
                raise ValueError(f"row_max_new must have one entry per row ({B}), got {len(row_max_new)}")
            lim = self.m._persistent("row_limits", (B,), torch.int32)
            lim.copy_(torch.as_tensor([int(v) for v in row_max_new], dtype=torch.int32))
            self.callback(set_limits, self.m._h, None, 0)
        _lib.check(set_limits(self.m._h, _lib.ptr(lim), B if lim is not None else 0), "itts_gpt_set_row_limits")
        return lim

    def chunk_return(self, k: int) -> None:
        """the early-return threshold of the chunk calls that follow; back to 0 when the owner closes"""
        if not self._resets_threshold:
            self.callback(_lib.lib().itts_gpt_set_chunk_return, self.m._h, 0)
            self._resets_threshold = True
        _lib.check(_lib.lib().itts_gpt_set_chunk_return(self.m._h, max(0, int(k))), "itts_gpt_set_chunk_return")


class UnifiedVoice:
    """`spk_cond_mode="campplus"` (IndexTTS-2.5, infer_v2_5.py:139): 3 conditioning tokens from the CAMPPlus style vector.
    Any other mode (IndexTTS-2, infer_v2.py:98; the reference default is "conformer"): 34 conditioning tokens -- 32 latents of
    the Conformer + Perceiver speaker encoder (`get_conditioning`, a prompt-side PyTorch module: set `conditioning_fn` or pass
    `conds_latent=`) plus the two `speed_emb` rows (model_v2.py:767-773); no language embedding (:680)."""
    _ALLOW_ENCODER_CONDITIONING = True

    def __init__(self, layers=8, model_dim=512, heads=8, max_text_tokens=120, max_mel_tokens=250,
                 max_conditioning_inputs=1, mel_length_compression=1024, number_text_tokens=256, start_text_token=0,
                 stop_text_token=1, number_mel_codes=8194, start_mel_token=8192, stop_mel_token=8193,
                 train_solo_embeddings=False, use_mel_codes_as_input=True, checkpointing=True, types=1,
                 condition_num_latent=32, condition_type="perceiver", condition_module=None, emo_condition_module=None,
                 use_accel=False, spk_cond_mode="conformer", precision="bf16", device="cuda:0", conditioning_fn=None, **_unused):
        self.conditioning_fn = conditioning_fn
        self.cond_num = condition_num_latent
        # Conformer + Perceiver conditioning encoders on the engine (indextts_amd/cond.py): built in load_state_dict when the config
        # carries their `condition_module` / `emo_condition_module` sections and the checkpoint their weights
        self.condition_type, self.condition_module, self.emo_condition_module = condition_type, condition_module, emo_condition_module
        self.cond_encoders = None
        self.layers, self.model_dim, self.heads = layers, model_dim, heads
        self.max_text_tokens, self.max_mel_tokens = max_text_tokens, max_mel_tokens
        self.max_conditioning_inputs = max_conditioning_inputs
        self.number_text_tokens, self.number_mel_codes = number_text_tokens, number_mel_codes
        self.start_text_token, self.stop_text_token = start_text_token, stop_text_token
        self.start_mel_token, self.stop_mel_token = start_mel_token, stop_mel_token
        self.types = types
        self.mel_length_compression = mel_length_compression
        self.spk_cond_mode = spk_cond_mode
        self.device = torch.device(device)
        self.precision = {"bf16": 1, "bfloat16": 1, "fp32": 0, "float32": 0, "f32": 0}[precision]
        self.kv_cache = True
        self.use_graph = True
        self.n_mel_pos = max_mel_tokens + 2 + max_conditioning_inputs
        self.n_text_pos = max_text_tokens + 2
        # `tts.gpt.text_pos_embedding.emb.num_embeddings` is read by the reference's text splitter (indextts/infer_v2_5.py:428) and
        # `mel_pos_embedding` likewise by callers sizing generation: attribute paths kept
        from types import SimpleNamespace
        self.text_pos_embedding = SimpleNamespace(emb=SimpleNamespace(num_embeddings=self.n_text_pos))
        self.mel_pos_embedding = SimpleNamespace(emb=SimpleNamespace(num_embeddings=self.n_mel_pos))
        cfg = _lib.GPTConfig()
        cfg.layers, cfg.model_dim, cfg.heads = layers, model_dim, heads
        cfg.vocab, cfg.n_mel_pos, cfg.precision = number_mel_codes, self.n_mel_pos, self.precision
        cfg.start_mel_token, cfg.stop_mel_token, cfg.ln_eps = start_mel_token, stop_mel_token, 1e-5
        self._h = C.c_void_p()
        with _lib.on_device(self.device):          # the handle (weights, stream, events) is bound to the device current here
            _lib.check(_lib.lib().itts_gpt_create(C.byref(cfg), C.byref(self._h)), "itts_gpt_create")
        self._emb: Dict[str, torch.Tensor] = {}
        self._loaded = False
        self._ws = None
        self._rescore_ws = None                # `rescore` owns a workspace of its own (a suspended loop lives in `_ws`)
        self._bufs = {}
        self.last_timing = None
        self.last_scores = None                      # `TokenScores` of the last generate(..., token_scores=True) call
        self.last_alignment = None                   # `TokenAlignment` of the last generate(..., alignment_heads=...) call
        self.last_prefix = None                      # dict(lens, chunks, decode_steps) of the last call that ingested a code prefix, else None

    # ---- checkpoint ------------------------------------------------------------------------------------------
    _ENGINE_PREFIXES = ("gpt.h.", "gpt.ln_f.", "final_norm.", "mel_head.")
    _HOST_TENSORS = ("mel_embedding.weight", "mel_pos_embedding.emb.weight", "text_embedding.weight",
                     "text_pos_embedding.emb.weight", "lang_embedding.weight", "spk_emb_proj.weight",
                     "spk_emb_proj.bias")

    _OPTIONAL_HOST_TENSORS = ("lang_embedding.weight",)

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = False):
        """Reference `gpt.pth` names (`strict=False` like indextts/utils/checkpoint.py:22-29); returns ignored keys."""
        L = _lib.lib()
        ignored = []
        for name, t in sd.items():
            if name in self._HOST_TENSORS:
                self._emb[name] = t.detach().to(self.device, torch.float32).contiguous()
            if name.startswith(self._ENGINE_PREFIXES) or name in ("mel_embedding.weight", "mel_pos_embedding.emb.weight"):
                if name.endswith(".attn.bias") or name.endswith(".attn.masked_bias"):
                    ignored.append(name)      # HF causal-mask buffers
                    continue
                tt = t.detach().to("cpu", torch.float32).contiguous()
                shape = (C.c_int64 * tt.dim())(*tt.shape)
                _lib.check(L.itts_gpt_load_tensor(self._h, name.encode(), C.c_void_p(tt.data_ptr()), shape, tt.dim()),
                           f"itts_gpt_load_tensor({name})")
            elif name not in self._HOST_TENSORS:
                ignored.append(name)
        _lib.check(L.itts_gpt_finalize(self._h), "itts_gpt_finalize")
        if "speed_emb.weight" in sd:
            self._emb["speed_emb.weight"] = sd["speed_emb.weight"].detach().to(self.device, torch.float32).contiguous()
        optional = set(self._OPTIONAL_HOST_TENSORS)
        if getattr(self, "spk_cond_mode", "campplus") != "campplus":          # IndexTTS-2: no style projection, speed embedding instead
            optional |= {"spk_emb_proj.weight", "spk_emb_proj.bias"}
            if type(self) is UnifiedVoice and "speed_emb.weight" not in self._emb:
                raise _lib.HipEngineError("UnifiedVoice.load_state_dict: missing ['speed_emb.weight']")
        missing = [n for n in self._HOST_TENSORS if n not in self._emb and n not in optional]
        if missing:
            raise _lib.HipEngineError(f"UnifiedVoice.load_state_dict: missing {missing}")
        emo_cm = getattr(self, "emo_condition_module", None)
        if emo_cm is not None and "emo_conditioning_encoder.after_norm.weight" in sd and "emovec_layer.weight" in sd:
            from .cond import ConditioningEncoders
            spk_cm = self.condition_module if (self.condition_type == "conformer_perceiver" and self.spk_cond_mode != "campplus"
                                                and "conditioning_encoder.after_norm.weight" in sd) else None
            self.cond_encoders = ConditioningEncoders(self.model_dim, spk_cm, emo_cm, cond_num=self.cond_num, device=self.device)
            self.cond_encoders.load_state_dict(sd)
            ignored = [n for n in ignored if not n.startswith(("emo_conditioning_encoder.", "emo_perceiver_encoder.", "emovec_layer.", "emo_layer."))
                       and not (spk_cm is not None and n.startswith(("conditioning_encoder.", "perceiver_encoder.")))]
        self._loaded = True
        return ignored

    def post_init_gpt2_config(self, use_deepspeed=False, kv_cache=False, half=False):
        """model_v2.py:422-493.  kv_cache=False reproduces the reference's no-cache position rule (positions 0..n-1)
        -- the engine always keeps a KV cache; only the mel position index changes."""
        self.kv_cache = bool(kv_cache)
        return self

    def eval(self):
        return self

    def to(self, device):
        """The engine lives on the device given at construction (`device=`); moving a loaded engine is not supported."""
        d = torch.device(device)
        if d.type == "cuda" and d.index is not None and self.device.index is not None and d.index != self.device.index:
            raise _lib.HipEngineError(f"UnifiedVoice was built on {self.device}; construct it with device={device!r} instead")
        return self

    # ---- input assembly (model_v2.py:648-714) ------------------------------------------------------------------
    def prepare_gpt_inputs(self, conditional_latents: torch.Tensor, text_inputs: torch.Tensor,
                           langs: Optional[torch.Tensor] = None):
        dev = self.device
        text_inputs = text_inputs.to(dev)
        conditional_latents = conditional_latents.to(dev, torch.float32)
        b, L = text_inputs.shape[:2]
        single_cond = conditional_latents.ndim == 3 and conditional_latents.shape[0] == 1
        if not single_cond:
            assert conditional_latents.shape[0] == b, f"batch size mismatch: {conditional_latents.shape[0]} vs {b}"
        n_cond = conditional_latents.shape[1]
        target_len = n_cond + L + 2
        valid = (text_inputs != self.stop_text_token) & (text_inputs != self.start_text_token)
        n_valid = valid.sum(dim=1)                                     # (b,)
        padding = L - n_valid                                           # left pad per row
        if L + 2 > self.n_text_pos and int(n_valid.max()) + 2 > self.n_text_pos:
            # the reference indexes text_pos_embedding out of range here (IndexError on CPU, device assert on a GPU)
            raise ValueError(f"text of {int(n_valid.max())} tokens exceeds max_text_tokens={self.max_text_tokens}")
        # gather valid ids to the right end of an (b, L+2) row: [pad..][start][ids][stop]
        order = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)          # valid ids first, in order
        ids_sorted = torch.gather(text_inputs.long(), 1, order)
        rows = torch.full((b, L + 2), self.stop_text_token, dtype=torch.long, device=dev)
        ar = torch.arange(L + 2, device=dev)[None, :]
        start_col = padding[:, None]
        rel = ar - start_col                                            # position within [start, ids..., stop]
        in_ids = (rel >= 1) & (rel <= n_valid[:, None])
        src = (rel - 1).clamp(0, L - 1)
        rows = torch.where(in_ids, torch.gather(ids_sorted, 1, src), rows)
        rows = torch.where(rel == 0, torch.full_like(rows, self.start_text_token), rows)
        tok_valid = rel >= 0
        pos = rel.clamp(min=0)
        emb = self._emb["text_embedding.weight"][rows] + self._emb["text_pos_embedding.emb.weight"][pos]
        if langs is not None and "lang_embedding.weight" in self._emb and getattr(self, "spk_cond_mode", "campplus") == "campplus":
            lg = langs.to(dev).long().reshape(-1)
            if lg.numel() == 1:
                lg = lg.expand(b)
            emb = emb + self._emb["lang_embedding.weight"][lg][:, None, :]
        emb = emb * tok_valid[..., None]                                # zero rows on the left pad
        cond = conditional_latents.expand(b, -1, -1) if single_cond else conditional_latents
        # [pad][cond][text]: roll the cond block to sit right after the pad
        out = torch.zeros(b, target_len, self.model_dim, dtype=torch.float32, device=dev)
        col = torch.arange(target_len, device=dev)[None, :]
        is_cond = (col >= padding[:, None]) & (col < padding[:, None] + n_cond)
        cond_idx = (col - padding[:, None]).clamp(0, n_cond - 1)
        out = torch.where(is_cond[..., None], torch.gather(cond, 1, cond_idx[..., None].expand(-1, -1, self.model_dim)), out)
        is_text = col >= padding[:, None] + n_cond
        text_idx = (col - n_cond).clamp(0, L + 1).expand(b, -1)
        out = torch.where(is_text[..., None], torch.gather(emb, 1, text_idx[..., None].expand(-1, -1, self.model_dim)), out)
        attention_mask = torch.ones(b, target_len + 1, dtype=torch.long, device=dev)
        attention_mask[:, :target_len] = (col >= padding[:, None]).long()
        fake_inputs = torch.ones(b, target_len + 1, dtype=torch.long, device=dev)
        fake_inputs[:, -1] = self.start_mel_token
        return fake_inputs, out, attention_mask

    def _spk_proj_params(self):
        """float64 host copies of spk_emb_proj's weight / bias, made once per loaded state dict (`_spk_proj`)"""
        w = self._emb["spk_emb_proj.weight"]
        hit = getattr(self, "_spk64", None)
        if hit is None or hit[0] is not w:
            hit = (w, w.detach().to("cpu", torch.float64), self._emb["spk_emb_proj.bias"].detach().to("cpu", torch.float64))
            self._spk64 = hit
        return hit[1], hit[2]

    def conds_latent(self, campplus_embedding: torch.Tensor, emo_vec: torch.Tensor) -> torch.Tensor:
        """spk_emb_proj(style) + emo_vec, then two zero tokens (model_v2.py:754-755,768)."""
        dev = self.device
        spk = _spk_proj(campplus_embedding.to(dev, torch.float32), *self._spk_proj_params())
        spk = spk.unsqueeze(0) if spk.ndim != 3 else spk
        emo_vec = emo_vec.to(dev, torch.float32)
        return torch.cat((spk + emo_vec.unsqueeze(1), torch.zeros(spk.size(0), 2, spk.size(2), device=dev)), 1), spk

    def get_conditioning(self, speech_conditioning_input, cond_mel_lengths=None):
        """IndexTTS-2 speaker latents (model_v2.py:556-586): Conformer + Perceiver -- on the engine when the checkpoint carried the
        encoders (`cond_encoders`), else through the injected `conditioning_fn` (e.g. the reference module's bound method)."""
        if self.conditioning_fn is not None:
            return self.conditioning_fn(speech_conditioning_input, cond_mel_lengths)
        if self.cond_encoders is not None and self.cond_encoders.spk is not None:
            if cond_mel_lengths is None:
                cond_mel_lengths = torch.full((speech_conditioning_input.shape[0],), speech_conditioning_input.shape[-1])
            return self.cond_encoders.get_conditioning(speech_conditioning_input, cond_mel_lengths)
        raise NotImplementedError("no conditioning encoder: load a checkpoint with conditioning_encoder.* / perceiver_encoder.* and a "
                                  "`condition_module` config, set UnifiedVoice.conditioning_fn, or pass conds_latent=")

    def get_emo_conditioning(self, speech_conditioning_input, cond_mel_lengths=None):        # model_v2.py:588-593
        self._need_cond("get_emo_conditioning")
        if cond_mel_lengths is None:
            cond_mel_lengths = torch.full((speech_conditioning_input.shape[0],), speech_conditioning_input.shape[-1])
        return self.cond_encoders.get_emo_conditioning(speech_conditioning_input, cond_mel_lengths)

    def get_emovec(self, emo_speech_conditioning_latent, emo_cond_lengths):                   # model_v2.py:827-831
        self._need_cond("get_emovec")
        return self.cond_encoders.get_emovec(emo_speech_conditioning_latent, emo_cond_lengths)

    def merge_emovec(self, speech_conditioning_latent, emo_speech_conditioning_latent, cond_lengths, emo_cond_lengths, alpha=1.0):
        self._need_cond("merge_emovec")                                                       # model_v2.py:833-838
        return self.cond_encoders.merge_emovec(speech_conditioning_latent, emo_speech_conditioning_latent, cond_lengths, emo_cond_lengths, alpha)

    def _need_cond(self, who):
        if self.cond_encoders is None:
            raise NotImplementedError(f"{who}: the checkpoint / config carried no emotion Conformer + Perceiver encoders "
                                      "(emo_condition_module, emo_conditioning_encoder.*, emo_perceiver_encoder.*, emovec_layer.*, emo_layer.*)")

    def conds_latent_v2(self, speech_conditioning_latent: torch.Tensor, emo_vec: torch.Tensor) -> torch.Tensor:
        """34 conditioning tokens of IndexTTS-2 (model_v2.py:767-773): latents + emo_vec, speed_emb(1), speed_emb(0)."""
        dev = self.device
        lat = speech_conditioning_latent.to(dev, torch.float32)
        se = self._emb["speed_emb.weight"]
        b = lat.shape[0]
        return torch.cat((lat + emo_vec.to(dev, torch.float32).unsqueeze(1), se[1].expand(b, 1, -1), se[0].expand(b, 1, -1)), 1)

    # ---- generation ----------------------------------------------------------------------------------------------
    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _persistent(self, name: str, shape, dtype) -> torch.Tensor:
        key = (name, tuple(int(v) for v in shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            if len(self._bufs) >= 32:
                self._bufs.clear()
            t = self._bufs[key] = torch.empty(*key[1], dtype=dtype, device=self.device)
        return t

    def _sync(self) -> None:
        """wait for the device work queued on torch's current stream: a setter that follows reads device memory back on the host"""
        torch.cuda.current_stream(self.device).synchronize()

    def _install_sampling(self, kind: str, entries) -> torch.Tensor:
        """the per-slot (kind "row") / the beam kernels' per-group (kind "group") sampling table on the device, installed on the engine handle
        (the caller uninstalls it: `_uninstall_sampling`)"""
        tab = self._persistent(f"{kind}_sampling", (len(entries), C.sizeof(type(entries[0]))), torch.uint8)   # its address is part of the graph key
        tab.copy_(_sampling_bytes(entries))
        self._sync()                                              # the engine reads the table back to check it
        what = f"itts_gpt_set_{kind}_sampling"
        _lib.check(getattr(_lib.lib(), what)(self._h, _lib.ptr(tab), len(entries)), what)
        return tab

    def _uninstall_sampling(self, kind: str):
        getattr(_lib.lib(), f"itts_gpt_set_{kind}_sampling")(self._h, None, 0)

    # (the two tables by name, as the tests of either one install them)
    def _install_row_sampling(self, entries) -> torch.Tensor:
        return self._install_sampling("row", entries)

    def _install_group_sampling(self, entries) -> torch.Tensor:
        return self._install_sampling("group", entries)

    def _uninstall_row_sampling(self):
        self._uninstall_sampling("row")

    def _uninstall_group_sampling(self):
        self._uninstall_sampling("group")

    def _logits_filters(self, kwargs: dict, inputs_embeds, max_new_tokens: int, num_beams: int, who: str):
        """`logits_filters` of a call's leftover generate kwargs, at this model's vocabulary and stop token and the call's prompt length
        (the cached prefix + the start-mel row: the length of the fake ids the reference hands to generate)"""
        return logits_filters(kwargs, self.number_mel_codes, self.stop_mel_token, int(max_new_tokens), num_beams, who,
                              prompt_len=int(inputs_embeds.shape[1]) + 1)

    def _filters_for(self, kwargs: dict, row_filters, group_filters, inputs_embeds, max_new_tokens: int, num_beams: int, who: str,
                     row_max_new=None):
        """What a decode entry installs for its filters: with `row_filters` (num_beams = 1) / `group_filters` (beam groups) the per-slot
        table (`_FilterTable`: `row_filter_entries` over the call's own filter kwargs), else the call-wide record of `_logits_filters`."""
        nb = int(num_beams)
        if row_filters is not None and nb != 1:
            raise ValueError(f"{who}: row_filters is the per-row table of num_beams = 1; beam groups take group_filters=")
        if group_filters is not None and nb == 1:
            raise ValueError(f"{who}: group_filters is the per-group table of the beam path (num_beams > 1); num_beams = 1 takes row_filters=")
        rows = row_filters if nb == 1 else group_filters
        if rows is None:
            return self._logits_filters(kwargs, inputs_embeds, max_new_tokens, nb, who)
        return _FilterTable(row_filter_entries(rows, int(inputs_embeds.shape[0]), kwargs, self.number_mel_codes, self.stop_mel_token,
                                               int(max_new_tokens), nb, who, prompt_len=int(inputs_embeds.shape[1]) + 1, row_max_new=row_max_new,
                                               name="row_filters" if nb == 1 else "group_filters"))

    def _install_filter_table(self, entries, slots: Optional[Sequence[int]] = None, n_slots: Optional[int] = None) -> None:
        """write `entries` into the engine's per-slot filter table (itts_gpt_set_row_filters): the whole table of len(entries) slots, or --
        slots given -- those slots of the installed table of n_slots"""
        n = len(entries)
        arr = (_lib.LogitsFilters * n)(*entries)          # (the records' arrays stay alive with `entries`; the engine copies them in the call)
        sl = None if slots is None else (C.c_int32 * n)(*[int(v) for v in slots])
        _lib.check(_lib.lib().itts_gpt_set_row_filters(self._h, arr, sl, n, n if n_slots is None else int(n_slots)), "itts_gpt_set_row_filters")

    def _install_filters(self, filt) -> None:
        """install the call's / session's logits filters on the engine handle -- a call-wide record, a `_FilterTable` or None: nothing to
        install; `_uninstall_filters` clears them"""
        if isinstance(filt, _FilterTable):
            self._install_filter_table(filt)
        elif filt is not None:
            _lib.check(_lib.lib().itts_gpt_set_logits_filters(self._h, C.byref(filt)), "itts_gpt_set_logits_filters")

    def _uninstall_filters(self, filt) -> None:
        if isinstance(filt, _FilterTable):
            _lib.lib().itts_gpt_set_row_filters(self._h, None, None, 0, 0)
        elif filt is not None:
            _lib.lib().itts_gpt_set_logits_filters(self._h, None)

    def _install_scores(self, B: int, max_new: int):
        """the call's / session's token-score arrays (logp_model, logp_sampled (B, max_new) f32) installed on the engine handle; persistent:
        their addresses are part of the decode graph's key.  The caller uninstalls them (`_uninstall_scores`)."""
        lm = self._persistent("logp_model", (B, max_new), torch.float32)
        ls = self._persistent("logp_sampled", (B, max_new), torch.float32)
        _lib.check(_lib.lib().itts_gpt_set_token_scores(self._h, _lib.ptr(lm), _lib.ptr(ls), B, max_new), "itts_gpt_set_token_scores")
        return lm, ls

    def _uninstall_scores(self):
        _lib.lib().itts_gpt_set_token_scores(self._h, None, None, 0, 0)

    def _code_prefix(self, code_prefix, code_prefix_lens, B: int, caps: Sequence[int], who: str):
        """The checked code prefix of a call's `code_prefix=` / `code_prefix_lens=`: -> (codes (B, W >= 1) int64 on the device, lens [B]),
        or None without one.  code_prefix: a (B, W) tensor (code_prefix_lens: the codes given per row, default W) or a list of B 1-D
        sequences (None / empty: a row without a prefix).  caps: each row's cap on its codes, which counts the prefix.  ValueError, never a
        silently different result: a prefix that holds the stop token (the row had ended), ids outside the code table, a prefix that leaves
        nothing to generate (len >= cap)."""
        if code_prefix is None:
            if code_prefix_lens is not None:
                raise ValueError(f"{who}: code_prefix_lens is given without code_prefix")
            return None
        if torch.is_tensor(code_prefix):
            if code_prefix.dim() != 2 or code_prefix.shape[0] != B:
                raise ValueError(f"{who}: code_prefix must be (B, W) with one row per prompt row ({B}) or a list of 1-D sequences, got {tuple(code_prefix.shape)}")
            W = int(code_prefix.shape[1])
            lens = [W] * B if code_prefix_lens is None else [int(v) for v in code_prefix_lens]
            rows = [code_prefix[b].detach().cpu().to(torch.int64) for b in range(B)]
        else:
            rows = [torch.zeros(0, dtype=torch.int64) if r is None else torch.as_tensor(r).detach().cpu().to(torch.int64).reshape(-1) for r in code_prefix]
            if len(rows) != B:
                raise ValueError(f"{who}: code_prefix must hold one sequence per prompt row ({B}), got {len(rows)}")
            lens = [int(r.numel()) for r in rows] if code_prefix_lens is None else [int(v) for v in code_prefix_lens]
        if len(lens) != B or any(k < 0 or k > int(r.numel()) for k, r in zip(lens, rows)):
            raise ValueError(f"{who}: code_prefix_lens must hold one entry per row ({B}) in 0 .. the row's width, got {lens}")
        for b, (k, r) in enumerate(zip(lens, rows)):
            p = r[:k]
            if bool((p == self.stop_mel_token).any()):
                raise ValueError(f"{who}: code_prefix of row {b} holds the stop token ({self.stop_mel_token}): the row had ended, there is nothing to continue")
            if bool(((p < 0) | (p >= self.number_mel_codes)).any()):
                raise ValueError(f"{who}: code_prefix of row {b} holds ids outside 0 .. {self.number_mel_codes - 1}")
            if k >= int(caps[b]):
                raise ValueError(f"{who}: code_prefix of row {b} holds {k} codes and the row's cap is {int(caps[b])}: the cap counts the prefix "
                                 "and must leave a code to generate")
        W = max(1, max(lens))
        pc = torch.zeros(B, W, dtype=torch.int64)
        for b, (k, r) in enumerate(zip(lens, rows)):
            pc[b, :k] = r[:k]
        return pc.to(self.device).contiguous(), lens

    @staticmethod
    def _prefix_caps(max_new: int, row_max_new, B: int, unit: str = "row") -> List[int]:
        """the caps a code prefix of `B` rows is checked against (`_code_prefix`): each row's own, min(max_new, row_max_new[b])"""
        if row_max_new is not None and len(row_max_new) != B:
            raise ValueError(f"row_max_new must have one entry per {unit} ({B}), got {len(row_max_new)}")
        return [int(max_new)] * B if row_max_new is None else [min(int(max_new), int(v)) for v in row_max_new]

    def _install_prefix(self, prefix, prefix_chunk: int, pos_offset: Optional[int] = None) -> None:
        """install a checked code prefix (`_code_prefix`) on the engine handle (itts_gpt_set_code_prefix); pos_offset: the position offset of
        the prefix embeddings (None: the decode step's own, the resume rule; 1: the reference's `input_tokens` prefill).  The caller
        uninstalls it (`_uninstall_prefix`)."""
        pc, lens = prefix
        chunk = int(prefix_chunk)
        if not 1 <= chunk <= 65535:
            raise ValueError(f"prefix_chunk must be in 1 .. 65535, got {chunk}")
        ppo = (2 if self.kv_cache else 1) if pos_offset is None else int(pos_offset)
        self._sync()                                              # the engine reads the codes back to check them
        _lib.check(_lib.lib().itts_gpt_set_code_prefix(self._h, _lib.ptr(pc), (C.c_int32 * len(lens))(*lens), len(lens), int(pc.shape[1]), ppo, chunk),
                   "itts_gpt_set_code_prefix")

    def _uninstall_prefix(self) -> None:
        _lib.lib().itts_gpt_set_code_prefix(self._h, None, None, 0, 0, 0, 0)

    def _record_prefix(self, lens, decode_steps: int) -> dict:
        """`last_prefix` of the call whose ingest just ran (itts_gpt_last_prefix): the record that the prefix was consumed -- a call whose
        engine ran no ingest raises here rather than return plain codes"""
        mx, ch = C.c_int32(0), C.c_int32(0)
        _lib.check(_lib.lib().itts_gpt_last_prefix(self._h, C.byref(mx), C.byref(ch)), "itts_gpt_last_prefix")
        if mx.value != max(lens):
            raise _lib.HipEngineError(f"code_prefix: the engine ingested a prefix of {mx.value} codes, the call gave {max(lens)}")
        self.last_prefix = dict(lens=[int(k) for k in lens], chunks=int(ch.value), decode_steps=int(decode_steps))
        return self.last_prefix

    def _alignment_request(self, heads, spans, inputs_embeds, who: str, num_beams: int = 1):
        """the checked (pairs, spans) of a call's `alignment_heads` / `text_spans`, or None without heads; host work only"""
        if heads is None:
            if spans is not None:
                raise ValueError(f"{who}: text_spans is given without alignment_heads")
            return None
        if num_beams != 1:
            raise ValueError(f"{who}: alignment_heads is implemented for num_beams = 1 only (a beam's rows change parents every step)")
        return alignment_pairs(heads, self.layers, self.heads, who), alignment_spans(spans, int(inputs_embeds.shape[0]), who)

    def _install_alignment(self, req, B: int, max_new: int, text_cap: Optional[int] = None):
        """the call's / session's alignment export installed on the engine handle: span (B, 2) int32 and out (B, max_new, K, text_cap) f32,
        persistent (their addresses are part of the decode graph's key).  The caller uninstalls it (`_uninstall_alignment`)."""
        pairs, spans = req
        cap = _alignment_text_cap(spans) if text_cap is None else int(text_cap)
        span = self._persistent("align_span", (B, 2), torch.int32)
        span.copy_(torch.as_tensor(spans, dtype=torch.int32).reshape(B, 2))
        out = self._persistent("align_out", (B, max_new, len(pairs), cap), torch.float32)
        flat = (C.c_int32 * (2 * len(pairs)))(*[v for p in pairs for v in p])
        _lib.check(_lib.lib().itts_gpt_set_alignment(self._h, flat, len(pairs), _lib.ptr(span), _lib.ptr(out), B, max_new, cap),
                   "itts_gpt_set_alignment")
        return span, out

    def _uninstall_alignment(self):
        _lib.lib().itts_gpt_set_alignment(self._h, None, 0, None, None, 0, 0, 0)

    def _prefix(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, nb: int = 1):
        """The engine's prompt of a generate call: the cached prefix (B, s, D) followed by the start-mel row -> x (B * nb, S, D) f32, pad
        (B * nb,) int32 (left-pad positions per row, from attention_mask (B, >= S)), S = s + 1.  nb > 1: every row repeated per beam, beams
        adjacent (_expand_inputs_for_generation)."""
        dev = self.device
        B, s, D = inputs_embeds.shape
        start = (self._emb["mel_embedding.weight"][self.start_mel_token] + self._emb["mel_pos_embedding.emb.weight"][0])
        x = torch.cat([inputs_embeds.to(dev, torch.float32), start.expand(B, 1, D)], dim=1)
        pad = (attention_mask[:, :s + 1] == 0).sum(dim=1).to(torch.int32).to(dev)
        if nb > 1:
            x, pad = x.repeat_interleave(nb, dim=0), pad.repeat_interleave(nb)
        return x.contiguous(), pad.contiguous(), s + 1

    def _penalty_ids(self):
        """the ids the repetition penalty has seen before the first token: the fake prefix ids (all ones) + start_mel"""
        return (C.c_int32 * 2)(1, self.start_mel_token)

    def _read_timing(self, compaction: bool = False) -> dict:
        """`last_timing` of the generate call that just returned (itts_gpt_last_timing); compaction: with the num_beams = 1 loop's row_steps
        (sum over the decode steps of the rows each step ran: B x steps when no row left the batch early) and compactions"""
        L = _lib.lib()
        pm, dm, st = C.c_float(0), C.c_float(0), C.c_int32(0)
        L.itts_gpt_last_timing(self._h, C.byref(pm), C.byref(dm), C.byref(st))
        self.last_timing = dict(prefill_ms=pm.value, decode_ms=dm.value, steps=st.value)
        if compaction:
            rs, nc = C.c_int64(0), C.c_int32(0)
            L.itts_gpt_compaction_stats(self._h, C.byref(rs), C.byref(nc))
            self.last_timing.update(row_steps=int(rs.value), compactions=int(nc.value))
        return self.last_timing

    def _beam_state(self, B: int, nb: int, max_new: int):
        """the buffers a beam call copies its search state to: hist_tok, hist_par (max_new, B * nb) i32, beam_scores (B * nb,) f32, hyps
        (B, 4, 4) f32 records {f32 score, i32 step, i32 row, pad}, n_hyps (B,) i32, done (B,) u8"""
        dev, nseq = self.device, B * nb
        return (torch.empty(max_new, nseq, dtype=torch.int32, device=dev), torch.empty(max_new, nseq, dtype=torch.int32, device=dev),
                torch.empty(nseq, dtype=torch.float32, device=dev), torch.empty(B, 4, 4, dtype=torch.float32, device=dev),
                torch.empty(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev))

    def _uniforms(self, uniforms, max_new: int, B: int):
        """the caller's (>= max_new_tokens, B) uniform stream in its persistent buffer (its address is part of the decode graph's key), or None"""
        if uniforms is None:
            return None
        if uniforms.shape[0] < max_new or uniforms.shape[1] != B:
            raise ValueError("uniforms must be (>= max_new_tokens, B)")
        u = self._persistent("uniforms", (max_new, B), torch.float64)
        u.copy_(uniforms[:max_new])
        return u

    @staticmethod
    def _seed(seed, do_sample, uniforms) -> int:
        """Device RNG seed.  `seed=None` (the default) draws it from torch's global generator, so sampled calls differ from
        call to call and follow `torch.manual_seed` like the reference's `torch.multinomial` does; an explicit seed is kept."""
        if seed is not None:
            return int(seed)
        if not do_sample or uniforms is not None:
            return 0
        return int(torch.randint(0, 2 ** 62, (1,)).item())

    def set_compaction(self, enable: bool = True, granularity: int = 8):
        """Row compaction of ragged decode batches (itts_gpt_set_compaction): finished rows leave the running batch in buckets of
        `granularity` rows.  On by default; results do not depend on it."""
        _lib.check(_lib.lib().itts_gpt_set_compaction(self._h, int(bool(enable)), int(granularity)), "itts_gpt_set_compaction")

    def graph_stats(self) -> dict:
        """decode-step hipGraphs captured / reused by this engine handle (itts_gpt_graph_stats)"""
        cap, hit = C.c_int32(0), C.c_int32(0)
        _lib.lib().itts_gpt_graph_stats(self._h, C.byref(cap), C.byref(hit))
        return dict(captures=cap.value, hits=hit.value)

    def generate(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int, do_sample=False,
                 num_beams=1, top_p=1.0, top_k=50, temperature=1.0, repetition_penalty=1.0, length_penalty=1.0,
                 uniforms: Optional[torch.Tensor] = None, seed: Optional[int] = None, typical_mass: float = 0.0,
                 row_max_new: Optional[Sequence[int]] = None, row_sampling: Optional[Sequence[dict]] = None,
                 group_sampling: Optional[Sequence[dict]] = None, token_scores: bool = False, alignment_heads=None, text_spans=None,
                 code_prefix=None, code_prefix_lens: Optional[Sequence[int]] = None, prefix_chunk: int = 128,
                 prefix_pos_offset: Optional[int] = None, row_filters: Optional[Sequence[Optional[dict]]] = None,
                 group_filters: Optional[Sequence[Optional[dict]]] = None, **unused) -> torch.Tensor:
        """`row_filters` (engine extension for mixed-request batches, num_beams = 1) / `group_filters` (num_beams > 1): one entry per row /
        utterance -- a dict of the logits-filter kwargs (`_LOGITS_FILTER_KWARGS`) or None -- merged over this call's own filter kwargs
        (`row_filter_entries`: the entry's key wins); the selection kernels then read their filters per slot (itts_gpt_set_row_filters).  A
        row decodes, bit for bit, as in the call whose call-wide filters are its merged kwargs; a row whose kwargs build nothing as in the
        plain call.  Installed for the call only, like the call-wide filters.  `no_repeat_ngram_size` stays a num_beams = 1 matter.
        `code_prefix` (engine extension, num_beams = 1; itts_gpt_set_code_prefix): continue every row after GIVEN codes -- a (B, W) tensor
        with `code_prefix_lens` (default W per row) or a list of B 1-D sequences (None: no prefix).  A row with prefix p[0 .. k) decodes as the
        row that had generated those k codes itself: its own step starts at k -- position embeddings, the draw (seed, stream, own step; a
        `uniforms` stream is read at the row's own step, so it keeps its full width), `max_new_tokens` / `row_max_new` (they count the
        prefix), the repetition penalty's set, the logits filters and the score / alignment columns (prefix columns hold 0.0).  The call
        returns the FULL rows, prefix included, and leaves `self.last_prefix = dict(lens, chunks, decode_steps)` (None after a call without
        a prefix).  The prefix runs through the stack `prefix_chunk` positions per pass (many-query kernels, as `rescore`): in exact
        arithmetic the continuation of a run's own prefix is that run's tail; in floating point its logits differ in the last bits from the
        decoded ones.  `prefix_pos_offset`: the position offset of the prefix embeddings (None: the decode step's, the resume rule; 1: the
        reference's `input_tokens` prefill, see `inference_speech`).  A prefix that holds the stop token, or leaves nothing to generate
        under the row's cap, raises ValueError.
        `alignment_heads=[(layer, head), ...]` with `text_spans=[(off, len), ...]` (engine extension, num_beams = 1): every decode step also
        writes the softmax weights of the selected heads over each row's text keys -- `len` keys from `off` after the row's first valid key
        (itts_gpt_set_alignment); the call leaves them in `self.last_alignment` (`TokenAlignment`, the columns of the returned ids; None without
        heads).  The returned ids are the same either way.
        `token_scores` (engine extension, num_beams = 1): the token selection also writes every stored token's log-probability under the
        model's own distribution and the one it was selected with (itts_gpt_set_token_scores); the call leaves them in `self.last_scores`
        (`TokenScores`, the columns of the returned ids; None when the flag is off).  The returned ids are the same either way.  HF's
        `output_scores` / `return_dict_in_generate` stay ignored: they would change the return type.
        `group_sampling` (engine extension, num_beams > 1): `row_sampling` for beam groups -- one dict per utterance with the keys of
        `row_sampling` plus `length_penalty` (`group_sampling_entries`; missing keys = this call's scalars, `stream` = the utterance index);
        the beam kernels then read their settings per group (itts_gpt_set_group_sampling), beam search and beam-sample groups may share the
        batch, and with `row_max_new` every utterance searches up to its own cap (what `max_new_tokens` is to it alone).
        `row_sampling` (engine extension for mixed-request batches): one dict per row with that row's own do_sample / top_k / top_p /
        temperature / repetition_penalty / typical_mass / seed / stream (`row_sampling_entries`; missing keys = this call's scalars, `stream`
        = the row index) -- the token selection then reads its settings per row (itts_gpt_set_row_sampling); num_beams = 1 only.
        `row_max_new` (engine extension for merged batches): per-row cap on generated tokens -- row b emits the stop token from token
        index row_max_new[b] on, i.e. each request of a batch keeps its own `max_mel_tokens` (sampling / greedy only).
        `GPT2InferenceModel.generate` for greedy / multinomial sampling (typical_mass > 0: the reference's
        TypicalLogitsWarper sits between the repetition penalty and the warpers, model_v2.py:794-799).  inputs_embeds (B,s,D) = the cached prefix;
        attention_mask (B,s+1).  Returns generated ids (B, n) (what `output[:, trunc_index:]` is in the reference)."""
        if not self._loaded:
            raise RuntimeError("UnifiedVoice: load_state_dict() first")
        if token_scores and num_beams != 1:
            raise ValueError("generate: token_scores=True is implemented for num_beams = 1 only (a beam's per-token transition scores need "
                             "beam_indices, which the beam search does not expose)")
        _refuse_timestamps(unused, "generate")
        align = self._alignment_request(alignment_heads, text_spans, inputs_embeds, "generate", num_beams)
        altering = sorted(k for k in unused if k in _UNSUPPORTED_GENERATE_KWARGS and unused[k] is not None)
        if altering:             # the reference forwards these to HF `generate`, where they change the ids: never drop them silently
            raise NotImplementedError(f"generate: {altering} would change the generated ids and the device loop does not implement them "
                                      f"(supported: {_SUPPORTED_GENERATE_KWARGS})")
        filt = self._filters_for(unused, row_filters, group_filters, inputs_embeds, max_new_tokens, num_beams, "generate", row_max_new)
        if code_prefix is not None and num_beams != 1:
            raise NotImplementedError("generate: code_prefix is implemented for num_beams = 1 only (a beam group's rows would share the prefix "
                                      "and its scores: the beam entries refuse an installed prefix)")
        prefix = None
        if code_prefix is not None or code_prefix_lens is not None:
            B = int(inputs_embeds.shape[0])
            prefix = self._code_prefix(code_prefix, code_prefix_lens, B, self._prefix_caps(max_new_tokens, row_max_new, B), "generate")
            if uniforms is not None and int(uniforms.shape[0]) < int(max_new_tokens):      # a row reads the stream at its own step, prefix counted
                raise ValueError(f"generate: with code_prefix, uniforms keeps the full width ({int(max_new_tokens)} rows, row b reads rows "
                                 f"len_b .. of its column), got {int(uniforms.shape[0])}")
        self._check_idle("generate")
        self.last_scores = self.last_alignment = self.last_prefix = None
        with _HandleState(self) as own:          # sticky on the handle: cleared when the call is over
            own.filters(filt)
            own.prefix(prefix, prefix_chunk, prefix_pos_offset)
            return self._generate(inputs_embeds, attention_mask, max_new_tokens, do_sample, num_beams, top_p, top_k, temperature,
                                  repetition_penalty, length_penalty, uniforms, seed, typical_mass, row_max_new, row_sampling, group_sampling,
                                  bool(token_scores), align, prefix)

    def _generate(self, inputs_embeds, attention_mask, max_new_tokens, do_sample, num_beams, top_p, top_k, temperature, repetition_penalty,
                  length_penalty, uniforms, seed, typical_mass, row_max_new, row_sampling, group_sampling, token_scores=False, align=None,
                  prefix=None) -> torch.Tensor:
        """`generate` past its kwarg checks, with the call's logits filters (and code prefix) installed"""
        if num_beams != 1:
            if row_sampling is not None:
                raise NotImplementedError("generate: row_sampling (per-row sampling settings) is implemented for num_beams=1 only; "
                                          "beam groups take group_sampling= (entries with a length_penalty)")
            return self._generate_beam(inputs_embeds, attention_mask, max_new_tokens, do_sample, num_beams, top_p, top_k,
                                       temperature, repetition_penalty, length_penalty, uniforms, seed, typical_mass,
                                       row_max_new=row_max_new, group_sampling=group_sampling)
        if group_sampling is not None:
            raise ValueError("generate: group_sampling is the table of the beam path (num_beams > 1); num_beams = 1 takes row_sampling=")
        dev = self.device
        B, max_new = inputs_embeds.shape[0], int(max_new_tokens)
        x, pad, S = self._prefix(inputs_embeds, attention_mask)
        gp = _gen_params(self.kv_cache, max_new, self._seed(seed, do_sample, uniforms), do_sample, 1, top_p, top_k, temperature,
                         repetition_penalty, length_penalty, typical_mass)
        L = _lib.lib()
        ws = self._workspace(L.itts_gpt_workspace_bytes(self._h, B, S, S + max_new))
        # output / uniforms buffers persist per shape: their addresses are part of the cached decode graph's key
        codes = self._persistent("codes", (B, max_new), torch.int64)
        n_steps = C.c_int32(0)
        u = self._uniforms(uniforms, max_new, B)
        entries = None if row_sampling is None else row_sampling_entries(row_sampling, B, _gp_defaults(gp))
        with _HandleState(self) as own:
            own.row_limits(row_max_new, B)
            own.sampling("row", entries)
            sc = own.scores(token_scores, B, max_new)
            al = own.alignment(align, B, max_new)
            rc = L.itts_gpt_generate(self._h, _lib.ptr(x), _lib.ptr(pad), B, S, C.byref(gp), self._penalty_ids(), 2, _lib.ptr(u),
                                     _lib.ptr(codes), C.byref(n_steps), _lib.ptr(ws), ws.numel(), int(self.use_graph),
                                     _lib.stream_ptr(self.device))
        _lib.check(rc, "itts_gpt_generate")
        self._read_timing(compaction=True)
        # HF stops right after the step at which every row has emitted EOS
        is_stop = codes == self.stop_mel_token
        first = torch.where(is_stop.any(1), is_stop.int().argmax(1) + 1, torch.full((B,), codes.shape[1], device=dev))
        n = int(min(int(first.max().item()), n_steps.value))
        starts = None
        if prefix is not None:                       # the shared step counter starts at 0 for every row: a row's columns run lens[b] ahead of it
            starts = prefix[1]
            self._record_prefix(starts, n_steps.value - 1)
            n = int(min(int(first.max().item()), n_steps.value + max(starts), max_new))
        if sc is not None or al is not None:
            lengths, ended = TokenScores.lengths_of(codes, [max_new] * B if row_max_new is None else [int(v) for v in row_max_new], self.stop_mel_token)
        if sc is not None:
            self.last_scores = TokenScores(sc[0][:, :n].clone(), sc[1][:, :n].clone(), lengths, ended, starts)
        if al is not None:
            self.last_alignment = TokenAlignment(al[1][:, :n].clone(), [l for _, l in align[1]], lengths)
        return codes[:, :n].clone()

    def rescore(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, codes: torch.Tensor, code_lens: Optional[Sequence[int]] = None,
                alignment_heads=None, text_spans=None, chunk: int = 128):
        """Teacher-forced second pass over GIVEN codes (itts_gpt_rescore; engine extension): the per-token log-probabilities and, with
        `alignment_heads=[(layer, head), ...]` / `text_spans=[(off, len), ...]`, the text attention that `generate(token_scores=True,
        alignment_heads=...)` exports at num_beams = 1 -- for ANY codes: a beam search's result, codes kept from an earlier call, codes of
        another checkpoint or precision.  inputs_embeds (B, s, D) / attention_mask (B, >= s + 1): the prompt as `generate` takes it; codes
        (B, W) int64; code_lens (B,): the codes scored per row, None = up to and including each row's first stop token
        (`TokenScores.lengths_of`).  Position i's input is the decode step's (mel_emb[code i - 1] + mel_pos[i - 1 + pos_offset]); `chunk`
        positions run per pass, so the cost in memory follows `chunk`, not W.  Leaves and returns (`last_scores`, `last_alignment`):
        `TokenScores` with logp_model (B, W) only (logp_sampled is None: nothing was selected) and `TokenAlignment` (None without heads), zero
        from code_lens[b] on.  Row 0 of the alignment is the start-mel query's attention here -- the decode export leaves it zero.  The pass
        owns a workspace of its own: a `generate_chunks` loop or a session suspended on this engine continues unchanged."""
        if not self._loaded:
            raise RuntimeError("UnifiedVoice: load_state_dict() first")
        who = "rescore"
        if codes.dim() != 2 or codes.shape[0] != inputs_embeds.shape[0] or codes.shape[1] < 1:
            raise ValueError(f"{who}: codes must be (B, W >= 1) with one row per prompt row, got {tuple(codes.shape)} for B = {inputs_embeds.shape[0]}")
        chunk = int(chunk)
        if not 1 <= chunk <= 65535:
            raise ValueError(f"{who}: chunk must be in 1 .. 65535, got {chunk}")
        B, W = int(codes.shape[0]), int(codes.shape[1])
        align = None
        if alignment_heads is not None:
            align = (alignment_pairs(alignment_heads, self.layers, self.heads, who), alignment_spans(text_spans, B, who))
        elif text_spans is not None:
            raise ValueError(f"{who}: text_spans is given without alignment_heads")
        codes = codes.to(self.device, torch.int64).contiguous()
        if code_lens is None:
            lengths, ended = TokenScores.lengths_of(codes, [W] * B, self.stop_mel_token)
        else:
            lengths = torch.as_tensor([int(v) for v in code_lens], dtype=torch.int64)
            if lengths.numel() != B or bool(((lengths < 0) | (lengths > W)).any()):
                raise ValueError(f"{who}: code_lens must hold one entry in 0 .. {W} per row ({B}), got {lengths.tolist()}")
            c = codes.cpu()
            ended = torch.tensor([bool(n > 0 and int(c[b, n - 1]) == self.stop_mel_token) for b, n in enumerate(lengths.tolist())])
        x, pad, S = self._prefix(inputs_embeds, attention_mask)
        L = _lib.lib()
        nbytes = L.itts_gpt_rescore_workspace_bytes(self._h, B, S, W, chunk)
        if nbytes == 0:
            raise ValueError(f"{who}: shape out of range (B = {B}, prompt {S}, {W} codes, chunk {chunk})")
        if self._rescore_ws is None or self._rescore_ws.numel() < nbytes:      # never the shared workspace: a suspended loop lives there
            self._rescore_ws = None
            self._rescore_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        ws = self._rescore_ws
        logp = torch.empty(B, W, dtype=torch.float32, device=self.device)
        lens = (C.c_int32 * B)(*[int(v) for v in lengths.tolist()])
        flat, span, out, cap, K = None, None, None, 0, 0
        if align is not None:
            pairs, spans = align
            K, cap = len(pairs), _alignment_text_cap(spans)
            flat = (C.c_int32 * (2 * K))(*[v for p in pairs for v in p])
            span = torch.as_tensor(spans, dtype=torch.int32).reshape(B, 2).to(self.device)
            out = torch.empty(B, W, K, cap, dtype=torch.float32, device=self.device)
        rc = L.itts_gpt_rescore(self._h, _lib.ptr(x), _lib.ptr(pad), B, S, _lib.ptr(codes), lens, W, 2 if self.kv_cache else 1, _lib.ptr(logp),
                                flat, K, _lib.ptr(span), _lib.ptr(out), cap, chunk, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(self.device))
        _lib.check(rc, "itts_gpt_rescore")
        self.last_scores = TokenScores(logp, None, lengths, ended)
        self.last_alignment = None if align is None else TokenAlignment(out, [l for _, l in align[1]], lengths)
        return self.last_scores, self.last_alignment

    def inference_speech_rescore(self, speech_condition, text_inputs, codes, langs=None, cond_lengths=None, emo_vec=None, campplus_embedding=None,
                                 conds_latent=None, code_lens=None, alignment_heads=None, text_spans=None, chunk: int = 128):
        """`rescore` behind the conditioning arguments of `inference_speech`: the prompt is built as `inference_speech` builds it
        (`_prepare_inference`), and with `alignment_heads` the text spans are derived as there.  -> (`TokenScores`, `TokenAlignment` or None)"""
        hf = {} if alignment_heads is None else dict(alignment_heads=alignment_heads, text_spans=text_spans)
        inputs_embeds, attention_mask, _, hf, _ = self._prepare_inference(speech_condition, text_inputs, langs, cond_lengths, emo_vec,
                                                                          campplus_embedding, None, 1, None, False, .9, conds_latent, hf)
        return self.rescore(inputs_embeds, attention_mask, codes, code_lens=code_lens, alignment_heads=alignment_heads,
                            text_spans=hf.get("text_spans"), chunk=chunk)

    def generate_chunks(self, inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int, chunk_size: int,
                        overlap_size: int, do_sample=False, num_beams=1, top_p=1.0, top_k=50, temperature=1.0, repetition_penalty=1.0,
                        length_penalty=1.0, uniforms: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                        typical_mass: float = 0.0, row_sampling: Optional[Sequence[dict]] = None, token_scores: bool = False,
                        alignment_heads=None, text_spans=None, code_prefix=None, code_prefix_lens: Optional[Sequence[int]] = None,
                        prefix_chunk: int = 128, prefix_pos_offset: Optional[int] = None,
                        row_filters: Optional[Sequence[Optional[dict]]] = None, **unused):
        """`row_filters`: per-row logits filters as in `generate`; the table stays installed over the chunk calls.
        `code_prefix` / `code_prefix_lens` / `prefix_chunk`: as in `generate`; the chunks cover the FULL rows from column 0 on (a row's
        prefix comes out with the first chunks), `self.last_prefix` is set by the first chunk call.
        `token_scores`: as in `generate`; `self.last_scores` holds the scores of every code generated so far after each chunk.
        `alignment_heads` / `text_spans`: as in `generate`; `self.last_alignment` likewise covers every code generated so far.
        Streaming form of `generate` (`GPTTRTEngine.generate_chunks`, backends/trt/runtime/gpt_trtllm_runtime.py:381-520):
        yields `(chunk_codes (B, <= chunk_size), is_last, batch_done [B], chunk_code_lens (B,))` as soon as `chunk_size` codes
        exist, consecutive chunks overlapping by `overlap_size` codes; the decode loop is suspended between chunks with its whole
        state (KV cache, position, finished flags) on the device (`itts_gpt_generate_chunk`).  Sampling / greedy only: the engine
        streams one hypothesis per row.  `row_sampling`: per-row sampling settings as in `generate`."""
        stride = int(chunk_size) - int(overlap_size)
        if stride <= 0:
            raise ValueError(f"overlap_size ({overlap_size}) must be less than chunk_size ({chunk_size}); "
                             f"got stride={stride} which would cause an infinite loop.")
        if num_beams != 1:
            if row_sampling is not None:
                raise NotImplementedError("generate_chunks: row_sampling is implemented for num_beams=1 only")
            if token_scores:
                raise ValueError("generate_chunks: token_scores=True is implemented for num_beams = 1 only")
            if alignment_heads is not None:
                raise ValueError("generate_chunks: alignment_heads is implemented for num_beams = 1 only")
            raise NotImplementedError("generate_chunks streams num_beams=1 (a beam's prefix is not final until the search ends)")
        if not self._loaded:
            raise RuntimeError("UnifiedVoice: load_state_dict() first")
        _refuse_timestamps(unused, "generate_chunks")
        prefix = None
        if code_prefix is not None or code_prefix_lens is not None:
            B = int(inputs_embeds.shape[0])
            prefix = self._code_prefix(code_prefix, code_prefix_lens, B, self._prefix_caps(max_new_tokens, None, B), "generate_chunks")
        align = self._alignment_request(alignment_heads, text_spans, inputs_embeds, "generate_chunks")
        # the suspended loop's state (KV cache in the workspace, the persistent `codes` buffer) is shared with generate(): another
        # generation on this object while a stream is open would corrupt it -> refuse until the stream is exhausted / closed
        self._check_idle("generate_chunks")
        filt = self._filters_for(unused, row_filters, unused.get("group_filters"), inputs_embeds, max_new_tokens, 1, "generate_chunks")
        self._stream_open = True
        self.last_scores = self.last_alignment = self.last_prefix = None
        try:
            with _HandleState(self) as own:     # everything stays installed over the chunk calls, for the generator's life
                own.filters(filt)
                own.prefix(prefix, prefix_chunk, prefix_pos_offset)      # consumed by the first chunk call (a resumed loop has its rows)
                yield from self._generate_chunks_body(own, inputs_embeds, attention_mask, max_new_tokens, chunk_size, overlap_size, stride, do_sample,
                                                      top_p, top_k, temperature, repetition_penalty, length_penalty, uniforms, seed, typical_mass,
                                                      row_sampling, bool(token_scores), align, prefix)
        finally:
            self._stream_open = False

    def _check_idle(self, who: str):
        if getattr(self, "_stream_open", False):
            raise RuntimeError(f"UnifiedVoice.{who}: a chunked generation (generate_chunks / infer_stream) is open on this engine; its "
                               "KV cache and code buffer live in the shared workspace.  Exhaust or close() that generator first, or use "
                               "a second UnifiedVoice for concurrent requests.")

    def _generate_chunks_body(self, own: _HandleState, inputs_embeds, attention_mask, max_new_tokens, chunk_size, overlap_size, stride, do_sample,
                              top_p, top_k, temperature, repetition_penalty, length_penalty, uniforms, seed, typical_mass, row_sampling=None,
                              token_scores=False, align=None, prefix=None):
        """the chunk loop of `generate_chunks`; own: that call's handle state, which this installs its tables into"""
        dev = self.device
        B, max_new = inputs_embeds.shape[0], int(max_new_tokens)
        x, pad, S = self._prefix(inputs_embeds, attention_mask)
        gp = _gen_params(self.kv_cache, max_new, self._seed(seed, do_sample, uniforms), do_sample, 1, top_p, top_k, temperature,
                         repetition_penalty, length_penalty, typical_mass)
        L = _lib.lib()
        ws = self._workspace(L.itts_gpt_workspace_bytes(self._h, B, S, S + max_new))
        codes = self._persistent("codes", (B, max_new), torch.int64)
        u = self._uniforms(uniforms, max_new, B)
        pen = self._penalty_ids()
        own.sampling("row", None if row_sampling is None else row_sampling_entries(row_sampling, B, _gp_defaults(gp)))
        sc = own.scores(token_scores, B, max_new)
        al = own.alignment(align, B, max_new)
        n_steps = C.c_int32(0)
        next_chunk_at = int(chunk_size)
        first = True
        while True:
            limit = min(next_chunk_at, max_new)
            rc = L.itts_gpt_generate_chunk(self._h, _lib.ptr(x) if first else None, _lib.ptr(pad), B, S, C.byref(gp), pen, 2, _lib.ptr(u),
                                           _lib.ptr(codes), limit, C.byref(n_steps), _lib.ptr(ws), ws.numel(), int(self.use_graph),
                                           _lib.stream_ptr(self.device))
            _lib.check(rc, "itts_gpt_generate_chunk")
            steps = int(n_steps.value)
            if prefix is not None:
                # every row's columns run lens[b] ahead of the shared step counter: row b holds own[b] = steps + lens[b] codes so far, and the
                # columns past them still hold the stop token the code rows are filled with -- they are not the row's stop token
                if first:
                    self._record_prefix(prefix[1], steps - 1)
                else:
                    self.last_prefix["decode_steps"] = steps - 1
                own = (torch.as_tensor(prefix[1], device=dev) + steps).clamp(max=max_new)
                width = int(own.max().item())
                got = codes[:, :width]
                caps_now = own.tolist()
            else:
                own, width, got, caps_now = None, steps, codes[:, :steps], [max_new] * B
            first = False
            if sc is not None:
                self.last_scores = TokenScores(sc[0][:, :width].clone(), sc[1][:, :width].clone(), *TokenScores.lengths_of(got, caps_now, self.stop_mel_token),
                                               None if prefix is None else prefix[1])
            if al is not None:
                self.last_alignment = TokenAlignment(al[1][:, :width].clone(), [l for _, l in align[1]],
                                                     TokenScores.lengths_of(got, caps_now, self.stop_mel_token)[0])
            is_stop = got == self.stop_mel_token
            if own is not None:
                is_stop = is_stop & (torch.arange(width, device=dev)[None, :] < own[:, None])
            done = is_stop.any(1)
            lens = torch.where(done, is_stop.int().argmax(1), torch.full((B,), steps, device=dev) if own is None else own)      # codes before the stop token
            current_len = int(lens.max().item())
            done_l, lens_l = done.tolist(), lens.tolist()
            finished = all(done_l) or steps >= max_new or steps < limit
            ready_len = current_len
            if own is not None and not finished:
                # rows with different prefixes hold different numbers of codes at one step: a chunk leaves when every row that is still
                # generating has all of its columns (without a prefix those rows all hold `steps` codes: the longest row decides, as ever)
                growing = [n for d, n in zip(done_l, lens_l) if not d and n < max_new]
                ready_len = min(growing) if growing else current_len
            while ready_len >= next_chunk_at:
                pos = next_chunk_at - chunk_size
                yield (codes[:, pos:next_chunk_at].clone(), False, [d and n <= next_chunk_at for d, n in zip(done_l, lens_l)],
                       torch.tensor([max(0, min(n - pos, chunk_size)) for n in lens_l], dtype=torch.long, device=dev))
                next_chunk_at += stride
            if finished:
                pos = next_chunk_at - chunk_size
                if pos < current_len:
                    yield (codes[:, pos:current_len].clone(), True, [True] * B,
                           torch.tensor([max(0, n - pos) for n in lens_l], dtype=torch.long, device=dev))
                return

    # ---- beam search / beam-sample (num_beams > 1; the reference default is 3-beam beam-sample) ------------------------
    def _generate_beam(self, inputs_embeds, attention_mask, max_new_tokens, do_sample, num_beams, top_p, top_k, temperature,
                       repetition_penalty, length_penalty, uniforms, seed, typical_mass=0.0, row_max_new=None, group_sampling=None) -> torch.Tensor:
        """row_max_new: per-utterance caps on the search's steps -- the capped call is ONE itts_gpt_generate_beam_chunk over all max_new_tokens
        steps (the session entry is the one that takes `group_caps`), finalised per group with min(cap, steps run) as a session does.
        group_sampling: per-utterance settings, installed for the call (itts_gpt_set_group_sampling)."""
        dev = self.device
        nb, max_new = int(num_beams), int(max_new_tokens)
        B = inputs_embeds.shape[0]
        x, pad, S = self._prefix(inputs_embeds, attention_mask, nb)
        gp = _gen_params(self.kv_cache, max_new, self._seed(seed, _any_group_samples(do_sample, group_sampling), uniforms), do_sample, nb, top_p,
                         top_k, temperature, repetition_penalty, length_penalty, typical_mass)
        caps = None
        if row_max_new is not None:
            if len(row_max_new) != B:
                raise ValueError(f"row_max_new must have one entry per utterance ({B}), got {len(row_max_new)}")
            if any(int(v) < 1 for v in row_max_new):                  # a beam search runs at least its first step (as max_new_tokens >= 1)
                raise ValueError("generate: every row_max_new entry must be >= 1 on the beam path")
            if uniforms is not None:
                raise NotImplementedError("generate: row_max_new with num_beams > 1 runs on the session entry, which takes no `uniforms`; use `seed`")
            caps = [min(max_new, int(v)) for v in row_max_new]
        entries = None if group_sampling is None else group_sampling_entries(group_sampling, B, _gp_group_defaults(gp))
        L = _lib.lib()
        ws = self._workspace(L.itts_gpt_beam_workspace_bytes(self._h, B, nb, S, S + max_new))
        hist_tok, hist_par, beam_scores, hyps, n_hyps, done = self._beam_state(B, nb, max_new)
        n_steps = C.c_int32(0)
        pen = self._penalty_ids()
        u = None
        if uniforms is not None:
            if uniforms.dim() != 3 or uniforms.shape[0] < max_new or uniforms.shape[1] != B or uniforms.shape[2] != 2 * nb:
                raise ValueError("uniforms must be (>= max_new_tokens, B, 2*num_beams)")
            u = self._persistent("beam_uniforms", (max_new, B, 2 * nb), torch.float64)
            u.copy_(uniforms[:max_new])
        with _HandleState(self) as own:
            own.sampling("group", entries)
            if caps is None:
                what = "itts_gpt_generate_beam"
                rc = L.itts_gpt_generate_beam(self._h, _lib.ptr(x), _lib.ptr(pad), B, nb, S, C.byref(gp), pen, 2, _lib.ptr(u),
                                              _lib.ptr(hist_tok), _lib.ptr(hist_par), _lib.ptr(beam_scores), _lib.ptr(hyps),
                                              _lib.ptr(n_hyps), _lib.ptr(done), C.byref(n_steps), _lib.ptr(ws), ws.numel(),
                                              int(self.use_graph), _lib.stream_ptr(self.device))
            else:                   # the session entry's first chunk, run to the end: it stops when every group is done or at its cap
                what = "itts_gpt_generate_beam_chunk"
                L.itts_gpt_set_chunk_return(self._h, 0)
                rc = L.itts_gpt_generate_beam_chunk(self._h, _lib.ptr(x), _lib.ptr(pad), B, nb, S, C.byref(gp), pen, 2, (C.c_int32 * B)(*caps),
                                                    _lib.ptr(hist_tok), _lib.ptr(hist_par), _lib.ptr(beam_scores), _lib.ptr(hyps),
                                                    _lib.ptr(n_hyps), _lib.ptr(done), max_new, C.byref(n_steps), _lib.ptr(ws), ws.numel(),
                                                    int(self.use_graph), _lib.stream_ptr(self.device))
        _lib.check(rc, what)
        self._read_timing()
        # ---- BeamSearchScorer.finalize (transformers_beam_search.py:320-408) on the host, one group at a time ----
        ht, hp = hist_tok.cpu().numpy(), hist_par.cpu().numpy()
        bs = beam_scores.cpu().numpy()
        hy = hyps.cpu().numpy()
        nh, dn = n_hyps.cpu().numpy(), done.cpu().numpy()
        # the reference loop ends at the first step after which every utterance is done (or at max_length)
        steps_run = beam_steps_run(hy, nh, dn, int(n_steps.value))
        stop = self.stop_mel_token
        own = [steps_run] * B if caps is None else [min(c, int(n_steps.value)) for c in caps]     # (a group that is not done ran to its cap, or to the end)
        lp = [length_penalty] * B if entries is None else [float(e.length_penalty) for e in entries]   # the value the device scored the group's hypotheses with
        best = [finalize_beam_group(ht, hp, bs, hy, nh, dn, own[b], lp[b], group=b, num_beams=nb) for b in range(B)]
        lens = [len(t) for t in best]
        sent_max = min(max(lens) + 1, max_new)
        out = torch.full((B, sent_max), stop, dtype=torch.int64)
        for b, t in enumerate(best):
            out[b, : len(t)] = torch.tensor(t[:sent_max], dtype=torch.int64)
        return out.to(dev)

    def _prepare_inference(self, speech_condition, text_inputs, langs, cond_lengths, emo_vec, campplus_embedding, input_tokens,
                           num_return_sequences, max_generate_length, typical_sampling, typical_mass, conds_latent, hf_generate_kwargs):
        """Argument handling of `inference_speech` up to the `generate` call (model_v2.py:716-803).  input_tokens (b, s) / (s,): the
        reference's code prefix (model_v2_5.py:735-751) -- carried in the returned kwargs as `code_prefix` with `prefix_pos_offset = 1` (its
        prefill embeds [start, c_0 .. c_{s-1}] at positions 0 .. s) and `input_tokens_len = s`, which the caller pops; the returned
        max_new_tokens is then s + the cap on NEW tokens, since the engine's caps count the prefix."""
        if num_return_sequences != 1:
            raise NotImplementedError("num_return_sequences > 1 is not used by the v2.5 pipeline")
        if typical_sampling and not (typical_mass > 0.0 and typical_mass < 1.0):           # model_v2.py:796-797
            raise ValueError(f"`typical_mass` has to be a float > 0 and < 1, but is {typical_mass}")
        if conds_latent is None:
            if emo_vec is None:
                raise NotImplementedError("emo_vec=None needs the Conformer/Perceiver emotion encoder (PyTorch side): "
                                          "compute it with merge_emovec / get_emovec and pass emo_vec=")
            if self.spk_cond_mode == "campplus":
                if campplus_embedding is None:
                    raise ValueError("campplus mode requires campplus_embedding or wav")
                conds_latent, spk_lat = self.conds_latent(campplus_embedding, emo_vec)
            else:                                                   # IndexTTS-2 (model_v2.py:761,767-773)
                if speech_condition.ndim == 2:
                    speech_condition = speech_condition.unsqueeze(0)
                if cond_lengths is None:       # model_v2.py:761 passes the feature width; = "all frames valid" (clamped to the frame count)
                    cond_lengths = torch.tensor([min(int(speech_condition.shape[-1]), int(speech_condition.shape[1]))],
                                                device=speech_condition.device)
                spk_lat = self.get_conditioning(speech_condition.transpose(1, 2), cond_lengths)
                conds_latent = self.conds_latent_v2(spk_lat, emo_vec)
                langs = None
        else:
            spk_lat = conds_latent[:, :1] if self.spk_cond_mode == "campplus" else conds_latent[:, : self.cond_num]
        input_ids, inputs_embeds, attention_mask = self.prepare_gpt_inputs(conds_latent, text_inputs, langs)
        max_new = (self.max_mel_tokens - 1) if max_generate_length is None else int(max_generate_length)
        hf = dict(hf_generate_kwargs)
        _reject_logits_processor(hf)
        hf["typical_mass"] = float(typical_mass) if typical_sampling else 0.0
        if hf.get("alignment_heads") is not None and hf.get("text_spans") is None:
            # the text keys of a row, after its left padding: [cond x n_cond][start][ids][stop] -> off = n_cond, len = n_valid + 2
            ti = text_inputs.to(self.device)
            n_valid = ((ti != self.stop_text_token) & (ti != self.start_text_token)).sum(dim=1).tolist()
            hf["text_spans"] = [(int(conds_latent.shape[1]), int(v) + 2) for v in n_valid]
        if input_tokens is not None:
            it = torch.as_tensor(input_tokens)
            it = it[None] if it.dim() == 1 else it
            B = int(inputs_embeds.shape[0])
            if it.dim() != 2 or it.shape[0] not in (1, B):
                raise ValueError(f"inference_speech: input_tokens must be (b, s) or (s,) with b = 1 or the batch ({B}), got {tuple(it.shape)}")
            if hf.get("code_prefix") is not None:
                raise ValueError("inference_speech: input_tokens and code_prefix are two rules for the same prefix; give one")
            # HF counts these from the end of the prompt, which holds input_tokens there; the engine's filters count from the row's first code
            per_row = [e for name in ("row_filters", "group_filters") for e in (hf.get(name) or ()) if isinstance(e, dict)]
            counted = sorted(k for k in ("min_new_tokens", "begin_suppress_tokens", "exponential_decay_length_penalty")
                             if hf.get(k) is not None or any(e.get(k) is not None for e in per_row))
            if counted:
                raise ValueError(f"inference_speech: {counted} with input_tokens would count from the row's first code here, not from the end of "
                                 "input_tokens as in the reference")
            hf["code_prefix"] = it.expand(B, -1).to(torch.int64)
            hf["prefix_pos_offset"] = 1
            hf["input_tokens_len"] = int(it.shape[1])
            max_new += int(it.shape[1])
        return inputs_embeds, attention_mask, max_new, hf, spk_lat

    def inference_speech(self, speech_condition, text_inputs, langs=None, emo_speech_condition=None, cond_lengths=None,
                         emo_cond_lengths=None, emo_vec=None, use_speed=False, campplus_embedding=None, wav=None,
                         input_tokens=None, num_return_sequences=1, max_generate_length=None, typical_sampling=False,
                         typical_mass=.9, conds_latent=None, uniforms=None, **hf_generate_kwargs):
        """model_v2.py:716-825 (campplus conditioning).  Returns (codes, speech_conditioning_latent).
        input_tokens (b, s) or (s,): the reference's code prefix (model_v2_5.py:682,735-751) under the REFERENCE's rule -- prefix code j is
        embedded at mel position j + 1 and the first generated code at s + 2 -- which is not the tail of the plain run; `code_prefix=` (a
        `generate` kwarg) is the engine's own resume rule.  Returns the new codes only (`output[:, trunc_index:]`); `max_generate_length`
        caps them.  A `uniforms` stream keeps its full width: s + max_generate_length rows, the new codes read rows s .. ."""
        inputs_embeds, attention_mask, max_new, hf, spk_lat = self._prepare_inference(
            speech_condition, text_inputs, langs, cond_lengths, emo_vec, campplus_embedding, input_tokens, num_return_sequences,
            max_generate_length, typical_sampling, typical_mass, conds_latent, hf_generate_kwargs)
        k = int(hf.pop("input_tokens_len", 0))
        codes = self.generate(inputs_embeds, attention_mask, max_new, uniforms=uniforms, **hf)
        return (codes[:, k:] if k else codes), spk_lat

    def inference_speech_stream(self, speech_condition, text_inputs, chunk_size=100, overlap_size=20, langs=None, cond_lengths=None,
                                emo_vec=None, campplus_embedding=None, max_generate_length=None, typical_sampling=False,
                                typical_mass=.9, conds_latent=None, uniforms=None, **hf_generate_kwargs):
        """`inference_speech` whose generate call yields code chunks as they are decoded (see `generate_chunks`): returns the
        (inputs_embeds, attention_mask, max_new_tokens, generate kwargs) a `streaming.StreamingDecoder` feeds back to this engine."""
        inputs_embeds, attention_mask, max_new, hf, _ = self._prepare_inference(
            speech_condition, text_inputs, langs, cond_lengths, emo_vec, campplus_embedding, None, 1, max_generate_length,
            typical_sampling, typical_mass, conds_latent, hf_generate_kwargs)
        hf["uniforms"] = uniforms
        return inputs_embeds, attention_mask, max_new, hf

    def inference_speech_inflight(self, speech_condition, text_inputs, langs=None, cond_lengths=None, emo_vec=None, campplus_embedding=None,
                                  max_generate_length=None, typical_sampling=False, typical_mass=.9, conds_latent=None, slots=8,
                                  chunk_tokens=16, min_free=1, row_max_new: Optional[Sequence[int]] = None,
                                  row_sampling: Optional[Sequence[dict]] = None, code_prefix=None, prefix_chunk: int = 128, **hf_generate_kwargs):
        """`inference_speech` for MORE utterances than decode slots: `slots` rows decode at a time and, whenever rows have emitted their stop
        token, waiting utterances are prefilled into the freed slots (`DecodeSession.admit`) instead of waiting for the whole batch to drain --
        the in-flight batching of the reference's serving path (backends/trt/serving/triton_server.py:96-305, pipeline.py:459-548) as a
        scheduling loop around the engine's suspended decode loop.  A row's ids do not depend on the batch it runs in or on when it joins
        (greedy: bit for bit the ids of `inference_speech` over all utterances at once; sampling: slot- and row-step-keyed random stream).

        ONE session serves the whole call: every slot keeps its own cache position and its own step (position embedding, token cap), so an
        utterance can join at any step with its full budget (`max_generate_length`, or its `row_max_new` cap) -- nothing of the session is
        bounded by the mel position table, only each row is.  Rows are polled every `chunk_tokens` tokens; an admission (one prefill launch
        train for all the utterances it places) waits until `min_free` slots are free -- or nothing is running.  `row_max_new`: per-utterance
        token caps as in `generate`; `row_sampling`: per-utterance sampling settings as in `generate` (one dict per utterance; give `stream` and
        `seed` to make an utterance's ids independent of the slot it lands in).  Returns (codes (N, L) padded with the stop token, speech_conditioning_latent); `last_inflight` holds the
        schedule's counters.  `token_scores=True` (a `generate` kwarg): `last_scores` holds the utterances' `TokenScores`, in utterance
        order, over the columns of the returned codes.  num_beams = 1.
        `code_prefix`: one sequence of given codes (or None) per utterance, as `generate(code_prefix=)`: the utterance is placed with its
        prefix (first batch or admission), its caps count it and it comes back as its full row.
        `row_filters` (through **hf_generate_kwargs): one entry per utterance as `generate(row_filters=)`; the session installs an
        utterance's entry into whatever slot it places it in."""
        emb, mask, max_new, hf, spk_lat = self._prepare_inference(
            speech_condition, text_inputs, langs, cond_lengths, emo_vec, campplus_embedding, None, 1, max_generate_length, typical_sampling,
            typical_mass, conds_latent, hf_generate_kwargs)
        if hf.get("num_beams", 1) != 1:
            raise NotImplementedError("inference_speech_inflight: num_beams = 1 only")
        if code_prefix is not None:
            if torch.is_tensor(code_prefix):
                code_prefix = [r for r in code_prefix]
            if all(p is None or len(p) == 0 for p in code_prefix):
                code_prefix = None
            else:
                hf["prefix_chunk"] = int(prefix_chunk)
        def harvest(sess, owner, cap):                      # one device reduction + one host synchronisation per poll
            out = []
            for b, n_codes in sess.finished_lengths():
                if owner[b] is not None:
                    c = sess._codes[b, :min(n_codes, cap[owner[b]])].clone()
                    out.append((b, c, c.numel() >= cap[owner[b]]) +       # ran into its cap before a stop token of its own
                               ((sess.scores(b),) if scored else ()) +     # ... and the row's token scores with it
                               ((sess.alignment(b),) if spans is not None else ()))      # ... and its text attention
            return out
        scored = bool(hf.get("token_scores"))
        self.last_scores = self.last_alignment = None
        spans = hf.pop("text_spans", None)                  # per utterance: handed to the session with the utterances it places
        if hf.get("alignment_heads") is not None:
            alignment_pairs(hf["alignment_heads"], self.layers, self.heads, "inference_speech_inflight")
            spans = alignment_spans(spans, emb.shape[0], "inference_speech_inflight")
            hf["alignment_text_cap"] = _alignment_text_cap(spans)          # one output array serves every utterance of the schedule
        if row_sampling is not None and len(row_sampling) != emb.shape[0]:
            raise ValueError(f"row_sampling must have one entry per utterance ({emb.shape[0]}), got {len(row_sampling)}")
        filters = self._inflight_filters(hf, "row_filters", "group_filters", emb.shape[0], "inference_speech_inflight")
        codes = self._inflight_schedule("inference_speech_inflight", emb, mask, max_new, hf, slots, chunk_tokens, min_free, row_max_new, harvest,
                                        lambda e, m, caps, rs=None, **kw: DecodeSession(self, e, m, max_new, row_max_new=caps, row_sampling=rs, **hf, **kw),
                                        row_sampling=row_sampling, text_spans=spans, code_prefix=code_prefix, filters=filters)
        return codes, spk_lat

    def inference_speech_inflight_beams(self, speech_condition, text_inputs, langs=None, cond_lengths=None, emo_vec=None, campplus_embedding=None,
                                        max_generate_length=None, typical_sampling=False, typical_mass=.9, conds_latent=None, slots=4,
                                        chunk_tokens=16, min_free=1, row_max_new: Optional[Sequence[int]] = None, num_beams=3,
                                        group_sampling: Optional[Sequence[dict]] = None, **hf_generate_kwargs):
        """`inference_speech_inflight` for beam search / beam-sample (the reference's default `num_beams=3`): `slots` beam GROUPS (one
        utterance's `num_beams` rows each) search at a time in one `BeamDecodeSession`; a group that is done -- or has reached its cap
        (`row_max_new`, else `max_generate_length`) -- is finalised on the host (`finalize_beam_group`) and its slot is refilled with a waiting
        utterance (`BeamDecodeSession.admit`) while the other groups keep searching.  The same scheduling loop, arguments, return value and
        `last_inflight` counters as `inference_speech_inflight`.  Beam search (`do_sample=False`): bit for bit the ids of
        `inference_speech(num_beams=...)` over all utterances at once; beam-sample: slot- and own-step-keyed random stream.
        `group_sampling`: per-utterance settings as in `generate` (one dict per utterance; give `stream` and `seed` to make an utterance's ids
        independent of the slot it lands in).  `group_filters` (through **hf_generate_kwargs): one entry per utterance as
        `generate(group_filters=)`; the session installs an utterance's entry into whatever group slot it places it in."""
        emb, mask, max_new, hf, spk_lat = self._prepare_inference(
            speech_condition, text_inputs, langs, cond_lengths, emo_vec, campplus_embedding, None, 1, max_generate_length, typical_sampling,
            typical_mass, conds_latent, hf_generate_kwargs)
        nb = int(num_beams)
        if nb < 2:
            raise ValueError("inference_speech_inflight_beams: num_beams >= 2 (inference_speech_inflight serves num_beams = 1)")
        if row_max_new is not None and any(int(v) < 1 for v in row_max_new):       # a beam search runs at least its first step (as max_new_tokens >= 1)
            raise ValueError("inference_speech_inflight_beams: every row_max_new entry must be >= 1")

        def harvest(sess, owner, cap):
            return [(b, sess.result(b), not sess.done(b)) for b in sess.finished() if owner[b] is not None]
        if group_sampling is not None and len(group_sampling) != emb.shape[0]:
            raise ValueError(f"group_sampling must have one entry per utterance ({emb.shape[0]}), got {len(group_sampling)}")
        filters = self._inflight_filters(hf, "group_filters", "row_filters", emb.shape[0], "inference_speech_inflight_beams")
        codes = self._inflight_schedule("inference_speech_inflight_beams", emb, mask, max_new, hf, slots, chunk_tokens, min_free, row_max_new, harvest,
                                        lambda e, m, caps, gs=None, **kw: BeamDecodeSession(self, e, m, max_new, num_beams=nb, row_max_new=caps,
                                                                                            group_sampling=gs, **hf, **kw),
                                        row_sampling=group_sampling, sampling_kw="group_sampling", filters=filters, filters_kw="group_filters")
        return codes, spk_lat

    @staticmethod
    def _inflight_filters(hf: dict, mine: str, other: str, n: int, who: str):
        """pop the per-utterance filter entries (`mine`: row_filters / group_filters) of an in-flight call from its generate kwargs"""
        if hf.pop(other, None) is not None:
            raise ValueError(f"{who}: {other} is the table of the {'beam path (num_beams > 1)' if other == 'group_filters' else 'num_beams = 1 path'}; "
                             f"this entry takes {mine}=")
        filters = hf.pop(mine, None)
        if filters is not None and len(filters) != n:
            raise ValueError(f"{mine} must have one entry per utterance ({n}), got {len(filters)}")
        return filters

    def _inflight_schedule(self, who, emb, mask, max_new, hf, slots, chunk_tokens, min_free, row_max_new, harvest, open_session, row_sampling=None,
                           sampling_kw="row_sampling", text_spans=None, code_prefix=None, filters=None, filters_kw="row_filters"):
        """The scheduling loop of `inference_speech_inflight` / `_beams`: `open_session(emb, mask, caps)` opens the session over the first
        `slots` utterances; `harvest(sess, owner, cap)` -> [(slot, ids before the stop token, ran into its cap[, the row's TokenScores])] of the
        finished slots that still hold an utterance (with scores: `last_scores` is left in utterance order).  row_sampling: per-utterance sampling dicts (beam sessions: group entries), handed to `open_session` as a
        fourth argument and to `admit(<sampling_kw>=)` for the utterances placed.  text_spans: per-utterance alignment spans, handed to
        `open_session(text_spans=)` and `admit(text_spans=)` likewise; harvested `TokenAlignment` rows are left in `last_alignment`.
        code_prefix: per-utterance given codes (a sequence or None each), handed to `open_session(code_prefix=)` and `admit(code_prefix=)`
        likewise: an utterance comes back as its full row, prefix included.  filters: per-utterance logits-filter entries, handed to
        `open_session(<filters_kw>=)` and `admit(<filters_kw>=)` likewise.  Returns codes (N, L) padded with the stop token; fills `last_inflight`."""
        N, slots, chunk = emb.shape[0], max(1, int(slots)), max(1, int(chunk_tokens))
        table = int(self._emb["mel_pos_embedding.emb.weight"].shape[0]) + 1 - (2 if self.kv_cache else 1)      # the engine's bound on a ROW's steps
        if max_new > table:
            raise ValueError(f"max_generate_length = {max_new} exceeds the mel position table ({table} steps)")
        stop = self.stop_mel_token
        if row_max_new is not None and len(row_max_new) != N:
            raise ValueError(f"row_max_new must have one entry per utterance ({N}), got {len(row_max_new)}")
        cap = [max_new if row_max_new is None else max(0, min(max_new, int(v))) for v in (row_max_new if row_max_new is not None else range(N))]
        caps_of = lambda idx: [cap[i] for i in idx]          # always enforced by the engine: a row at its cap emits the stop token (a beam group
                                                               # stops searching), which is what frees its slot (admission needs the engine to
                                                               # have the slot as finished)
        min_free = max(1, int(min_free))
        results: List[Optional[torch.Tensor]] = [None] * N
        scored: List[Optional[TokenScores]] = [None] * N
        aligned: List[Optional[TokenAlignment]] = [None] * N
        if code_prefix is not None and len(code_prefix) != N:
            raise ValueError(f"code_prefix must have one entry per utterance ({N}), got {len(code_prefix)}")
        sp_of = lambda idx: dict({} if text_spans is None else dict(text_spans=[text_spans[i] for i in idx]),      # what goes with the utterances
                                 **({} if code_prefix is None else dict(code_prefix=[code_prefix[i] for i in idx])),  # placed: spans, given codes,
                                 **({} if filters is None else {filters_kw: [filters[i] for i in idx]}))              # filter entries
        stats = dict(sessions=1, admitted=0, admissions=0, steps=0, row_steps=0, truncated=0)
        first, pending = list(range(N))[:slots], list(range(N))[slots:]
        B = len(first)
        owner: List[Optional[int]] = list(first)
        rs_of = lambda idx: [row_sampling[i] for i in idx]
        with (open_session(emb[first], mask[first], caps_of(first), **sp_of(first)) if row_sampling is None else
              open_session(emb[first], mask[first], caps_of(first), rs_of(first), **sp_of(first))) as sess:
            while any(o is not None for o in owner):
                before = sess.steps
                # while utterances wait, come back as soon as `min_free` slots can be refilled (the engine looks at its flags every few steps)
                sess.run(chunk, return_when_finished=min(min_free, len(pending), B) if pending else 0)
                stats["row_steps"] += (sess.steps - before) * sum(o is not None for o in owner)
                if sess.steps == before:
                    raise _lib.HipEngineError(f"{who}: the decode session made no progress")
                for b, c, truncated, *extra in harvest(sess, owner, cap):
                    for e in extra:
                        if isinstance(e, TokenScores):
                            scored[owner[b]] = e
                        else:
                            aligned[owner[b]] = e
                    if truncated:
                        stats["truncated"] += 1
                    if c.numel() < max_new:
                        c = torch.cat([c, c.new_full((1,), stop)])
                    results[owner[b]] = c
                    owner[b] = None
                free = [b for b in range(B) if owner[b] is None]
                enough = len(free) >= min(min_free, len(pending)) or len(free) == B
                if free and pending and enough:
                    take, pending = pending[:len(free)], pending[len(free):]
                    free = free[:len(take)]
                    sess.admit(free, emb[take], mask[take], row_max_new=caps_of(take), **({} if row_sampling is None else {sampling_kw: rs_of(take)}),
                               **sp_of(take))
                    for b, i in zip(free, take):
                        owner[b] = i
                    stats["admitted"] += len(take)
                    stats["admissions"] += 1
            stats["steps"] = sess.steps
        # slot_steps = steps x slots (on both the num_beams = 1 and the beam path).  row_steps charges a whole chunk to every slot that held an
        # utterance when the chunk started -- a row / group that finishes inside a chunk counts as live until it is harvested -- so
        # 1 - row_steps / slot_steps is a LOWER bound on the idle share of the session's slot-steps, not a measurement of it.
        stats["slot_steps"] = stats["steps"] * B
        self.last_inflight = stats
        width = max(int(c.numel()) for c in results)
        codes = torch.full((N, width), stop, dtype=torch.int64, device=self.device)
        for i, c in enumerate(results):
            codes[i, : c.numel()] = c
        if all(r is not None for r in scored):
            st = TokenScores.stack(scored)
            fit = lambda t: t[:, :width] if t.shape[1] >= width else F.pad(t, (0, width - t.shape[1]))     # the columns of `codes`
            self.last_scores = TokenScores(fit(st.logp_model), fit(st.logp_sampled), st.lengths, st.ended, st.starts)
        if all(r is not None for r in aligned):
            st = TokenAlignment.stack(aligned)
            a = st.attn[:, :width] if st.attn.shape[1] >= width else F.pad(st.attn, (0, 0, 0, 0, 0, width - st.attn.shape[1]))
            self.last_alignment = TokenAlignment(a, st.text_lens, st.lengths)
        return codes

    # ---- teacher-forced latent pass (model_v2.py:596-646) ----------------------------------------------------------
    def _latent_prefix(self, conds: torch.Tensor, text_inputs: torch.Tensor, text_lengths: torch.Tensor) -> torch.Tensor:
        """`conds | text_emb([start_text, ids, stop_text])` of the teacher-forced pass, (B, n_cond + L + 2, D): ids past a row's
        length become the stop text token (model_v2.py:610-617)."""
        dev = self.device
        text = text_inputs.to(dev).long().clone()
        tl = text_lengths.to(dev)
        text = torch.where(torch.arange(text.shape[1], device=dev)[None] >= tl[:, None],
                           torch.full_like(text, self.stop_text_token), text)
        text = F.pad(F.pad(text, (0, 1), value=self.stop_text_token), (1, 0), value=self.start_text_token)
        te = self._emb["text_embedding.weight"][text] + self._emb["text_pos_embedding.emb.weight"][: text.shape[1]]
        return torch.cat([conds.to(dev, torch.float32), te], dim=1)

    def latent_conds(self, speech_conditioning_latent, emo_vec, use_speed=None) -> torch.Tensor:
        """The conditioning block of `forward` (model_v2.py:634-637): IndexTTS-2's 34 tokens (latents + emo_vec, the two speed
        embeddings), or the campplus mode's projected latent + emo_vec followed by two zero rows."""
        dev = self.device
        spk = speech_conditioning_latent.to(dev, torch.float32)
        if self.spk_cond_mode != "campplus":
            se = self._emb["speed_emb.weight"]
            us = torch.zeros(spk.shape[0], dtype=torch.long, device=dev) if use_speed is None else torch.as_tensor(use_speed).to(dev).long()
            dur, half = se[torch.zeros_like(us)], se[torch.ones_like(us)]
            return torch.cat((spk + emo_vec.to(dev, torch.float32).unsqueeze(1), half.unsqueeze(1), dur.unsqueeze(1)), 1)
        return torch.cat((spk + emo_vec.to(dev, torch.float32).unsqueeze(1), torch.zeros(spk.size(0), 2, spk.size(2), device=dev)), 1)

    def latent_session(self, conds: torch.Tensor, text_inputs: torch.Tensor, text_lengths: torch.Tensor, max_codes: int,
                       max_append: int) -> "LatentSession":
        """A KV-cached teacher-forced pass (`itts_gpt_latent_open`): `append(codes_new)` returns the latents of the next mel
        positions at O(new positions) cost -- the per-chunk latent of streamed IndexTTS-2.  Every row runs at its OWN text length
        (`[start_text, ids[:text_lengths[b]], stop_text]`, no padding in between: what the pass gives the row alone).  The session
        owns its workspace, so it runs beside an open `generate_chunks` / `DecodeSession` on this engine."""
        return LatentSession(self, conds, text_inputs, text_lengths, max_codes, max_append)

    def forward_latent(self, conds: torch.Tensor, text_inputs: torch.Tensor, text_lengths: torch.Tensor,
                       mel_codes: torch.Tensor, mel_codes_lengths: torch.Tensor) -> torch.Tensor:
        self._check_idle("forward_latent")
        dev = self.device
        mel = mel_codes.to(dev).long().clone()
        ml = mel_codes_lengths.to(dev)
        mel = torch.where(torch.arange(mel.shape[1], device=dev)[None] >= ml[:, None],
                          torch.full_like(mel, self.stop_mel_token), mel)
        mel = F.pad(F.pad(mel, (0, 1), value=self.stop_mel_token), (1, 0), value=self.start_mel_token)
        me = self._emb["mel_embedding.weight"][mel] + self._emb["mel_pos_embedding.emb.weight"][: mel.shape[1]]
        x = torch.cat([self._latent_prefix(conds, text_inputs, text_lengths), me], dim=1).contiguous()
        B, S, D = x.shape
        L = _lib.lib()
        ws = self._workspace(L.itts_gpt_workspace_bytes(self._h, B, S, S))
        out = torch.empty_like(x)
        _lib.check(L.itts_gpt_forward_latent(self._h, _lib.ptr(x), B, S, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                             _lib.stream_ptr(self.device)), "itts_gpt_forward_latent")
        enc = out[:, conds.shape[1]:]
        return enc[:, -mel.shape[1]:][:, :-2]

    def forward(self, speech_conditioning_latent, text_inputs, text_lengths, mel_codes, mel_codes_lengths,
                emo_speech_conditioning_latent=None, cond_mel_lengths=None, emo_cond_mel_lengths=None, emo_vec=None,
                use_speed=None, do_spk_cond=False):
        """`UnifiedVoice.forward` of v2/v2.5 (model_v2.py:596-646; call site infer_v2.py:636-651): the teacher-forced
        pass that returns the mel-position latents.  campplus conditioning: `speech_conditioning_latent` is the style
        vector when `do_spk_cond` (projected here) or the projected (b,1,D) latent otherwise; `emo_vec` must be given
        (the emotion Conformer/Perceiver is outside this path)."""
        if emo_vec is None:
            raise NotImplementedError("emo_vec=None needs the emotion encoder (PyTorch side); pass emo_vec=")
        dev = self.device
        spk = speech_conditioning_latent.to(dev, torch.float32)
        if self.spk_cond_mode != "campplus":                       # IndexTTS-2: latents (b, 32, D) + speed embeddings (:634-637)
            if do_spk_cond:
                spk = self.get_conditioning(spk.transpose(1, 2), cond_mel_lengths).to(dev, torch.float32)
        elif do_spk_cond:
            spk = _spk_proj(spk, *self._spk_proj_params())
            if spk.ndim != 3:
                spk = spk.unsqueeze(1)
        return self.forward_latent(self.latent_conds(spk, emo_vec, use_speed), text_inputs, text_lengths, mel_codes, mel_codes_lengths)

    __call__ = forward

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._h.value:
                _lib.lib().itts_gpt_destroy(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass


def _session_init(init):
    """A session's __init__: the owner of what it installs on the engine handle (`_own`) is made first and closed on any exception out of
    `init`, so nothing of a session that did not open stays on the handle and `close()` never meets a half-built one; a session that did open
    marks the engine busy."""
    @functools.wraps(init)
    def opened(self, model: "UnifiedVoice", *args, **kwargs):
        self.m, self._own = model, _HandleState(model)
        try:
            init(self, model, *args, **kwargs)
        except BaseException:
            self._own.close()
            raise
        model._stream_open = True                    # the workspace holds this session's state until close()
    return opened


class _SessionBase:
    """What `DecodeSession` and `BeamDecodeSession` share: the prompt of the first batch, the session's counters, the admission workspace and
    the checks of `admit`, the per-slot sampling table's upkeep, `close` and the context manager.  The subclass names what a slot holds (`_UNIT`),
    what a slot that is not free is doing (`_BUSY`) and what its sampling table is per (`_PER`: the `<_PER>_sampling=` table)."""
    _UNIT = _BUSY = _PER = ""

    def _open(self, model: "UnifiedVoice", inputs_embeds, attention_mask, max_new_tokens: int, nb: int, gp):
        self.dev = model.device
        self.B, self.D, self.max_new = inputs_embeds.shape[0], inputs_embeds.shape[2], int(max_new_tokens)
        self._x, self._pad, self.S = model._prefix(inputs_embeds, attention_mask, nb)      # nb > 1: one row per beam, beams adjacent
        self._gp = gp
        self._pen = model._penalty_ids()
        self.steps = 0                               # steps of the session (= tokens generated by the rows of the first batch while they run)
        self.step0 = [0] * self.B                    # the session step of the own step 0 (first token) of the utterance currently in each slot
        self._first = True
        self._adm_ws = None
        self._tab = None                             # the installed per-slot sampling table, or None
        self._filt = None                            # the installed logits filters, or None

    @classmethod
    def _check_kwargs(cls, uniforms, unused):
        who = cls.__name__
        if uniforms is not None:        # a uniform stream is laid out per (step, row / utterance) of ONE batch; slots here change utterances
            raise NotImplementedError(f"{who}: `uniforms` is not supported ({cls._PER}s are re-occupied); use `seed`")
        _refuse_timestamps(unused, who)
        altering = sorted(k for k in unused if k in _UNSUPPORTED_GENERATE_KWARGS and unused[k] is not None)
        if altering:                    # as `generate`: never drop kwargs that change the ids silently
            raise NotImplementedError(f"{who}: {altering} would change the generated ids and the device loop does not implement them")

    def _open_filters(self, filt, kwargs: Optional[dict] = None):
        """install the session's logits filters (`UnifiedVoice._filters_for` of its leftover kwargs: the call-wide record or the per-slot
        table) until close(): the last step of __init__ before the session is open.  kwargs: the session's own filter kwargs, the defaults
        of the entries an admission brings."""
        self._filter_kwargs = {k: v for k, v in (kwargs or {}).items() if k in _LOGITS_FILTER_KWARGS}
        self._own.filters(filt)
        self._filt = filt

    def _free_slots_checked(self, sl: List[int]) -> List[int]:
        """`sl`, once every slot in it is in range, named once and finished (one `finished()` poll): the slots whose per-slot records the
        host may rewrite before the engine's admission call, which refuses the same slots before it touches anything"""
        fin = set(self.finished())
        bad = [v for v in sl if not 0 <= v < self.B or v not in fin]
        if bad or len(set(sl)) != len(sl):
            raise ValueError(f"{type(self).__name__}.admit: slots {bad or sl} are out of range, repeated or still {self._BUSY}")
        return sl

    def _admit_filters(self, sl: List[int], filters, prompt_len: int, row_max_new, nb: int) -> None:
        """`admit(<_PER>_filters=)`: the admitted utterances' entries -- merged over the session's own filter kwargs, at their own prompt
        length and caps -- into the slots they take.  A session opened with a table rewrites the slots at EVERY admission (no entries: the
        session's own kwargs), so a slot never keeps its previous occupant's filters; the kernels read a slot's record every step and the
        engine synchronises its stream before the rewrite.  The records are written BEFORE the engine's admission call: if that call then
        fails, the slots keep the new records -- harmless, since only finished slots are written (`sl` is `_free_slots_checked`), a finished
        slot's record is not read, and the next admission into the slot writes it again."""
        who, name = f"{type(self).__name__}.admit", f"{self._PER}_filters"
        if not isinstance(self._filt, _FilterTable):
            if filters is not None:
                raise ValueError(f"{who}: {name} needs a session opened with {name}= (the per-slot table is sized when the session opens)")
            return
        entries = row_filter_entries([None] * len(sl) if filters is None else filters, len(sl), self._filter_kwargs, self.m.number_mel_codes,
                                     self.m.stop_mel_token, self.max_new, nb, who, prompt_len=prompt_len, row_max_new=row_max_new, name=name)
        self.m._install_filter_table(entries, slots=sl, n_slots=self.B)

    def _next_limit(self, n: int, return_when_finished: int) -> int:
        """the step limit of the next chunk call of `n` steps; sets the engine's early-return threshold for it"""
        self._own.chunk_return(return_when_finished)
        return self.steps + int(n) if not self._first else min(self.max_new, int(n))

    def _admit_inputs(self, slots, inputs_embeds, attention_mask, row_max_new, sampling, caps_required: Optional[bool], workspace_bytes,
                      rewrites: bool = False):
        """`admit`'s argument checks; -> (x, pad, S_new, slots as a ctypes array, slots as ints) with the admission workspace grown to
        workspace_bytes(handle, n, S_new).  caps_required: whether row_max_new must (True) / must not (False) be given; None: optional.
        An admission that rewrites per-slot records on the host -- sampling entries, a session's filter table, or (rewrites) anything else
        -- gets its slots back `_free_slots_checked`: once, before any write."""
        who, per = f"{type(self).__name__}.admit", self._PER
        if self._first or self.steps < 1:
            raise RuntimeError(f"{who}: run() the first batch before admitting")
        n, s, D = inputs_embeds.shape
        if (sampling is not None) != (self._tab is not None):
            raise ValueError(f"{who}: {self._PER}_sampling must be given exactly when the session was opened with per-{per} sampling settings")
        if caps_required is not None and (row_max_new is not None) != caps_required:
            raise ValueError(f"{who}: row_max_new must be given exactly when the session was opened with per-row caps")
        if row_max_new is not None and len(row_max_new) != n:
            raise ValueError(f"row_max_new must have one entry per admitted {self._UNIT} ({n}), got {len(row_max_new)}")
        if len(slots) != n:
            raise ValueError(f"{who}: {len(slots)} slots for {n} utterances")
        if s + 1 > self.S:
            raise ValueError(f"{who}: the prompt ({s + 1} positions) is longer than the session's cache rows hold ({self.S})")
        x, pad, S_new = self.m._prefix(inputs_embeds, attention_mask)
        need = workspace_bytes(self.m._h, n, S_new)
        if self._adm_ws is None or self._adm_ws.numel() < need:
            self._adm_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
        sl = [int(v) for v in slots]
        if rewrites or sampling is not None or isinstance(self._filt, _FilterTable):
            sl = self._free_slots_checked(sl)
        return x, pad, S_new, (C.c_int32 * n)(*sl), sl

    def _rewrite_entries(self, sl: List[int], sampling, entries_of, defaults: dict) -> list:
        """The kernels read a slot's entry every step, so the entries of the finished slots `sl` (`_free_slots_checked`) are rewritten in
        stream order before the engine computes the new utterances' first token."""
        entries = entries_of(sampling, len(sl), defaults, slots=sl)
        self._tab[torch.as_tensor(sl, device=self.dev)] = _sampling_bytes(entries).to(self.dev)
        return entries

    def close(self):
        """clear everything the session installed on the engine handle and give the engine back; closing twice is harmless"""
        try:
            self._own.close()
        finally:
            self.m._stream_open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DecodeSession(_SessionBase):
    """A decode batch that keeps running while its utterances finish and NEW utterances are admitted into the freed slots (design reference: the
    in-flight batching of the reference's serving path, backends/trt/serving/triton_server.py:96-305, backends/trt/pipeline/pipeline.py:459-548).
    Built on the suspended-loop API of the engine: `run(n)` advances every live row by n tokens (`itts_gpt_generate_chunk`), `finished()` reports
    the slots whose row has emitted its stop token, `admit(slots, ...)` prefills new prompts into those slots (`itts_gpt_admit_rows`).  Every slot
    keeps its OWN cache position and its OWN step: an admitted utterance's keys sit at positions 0 .. of its cache row, its codes start at column
    0 of its code row, its position embeddings, random stream and token cap count from its first token -- so it generates, bit for bit, the ids
    it generates decoded alone, whatever step it joins at, and the session runs for as long as utterances keep arriving (only a ROW is bounded,
    by `max_new_tokens`).  Greedy / sampling, num_beams = 1.

    inputs_embeds (B, s, D) / attention_mask (B, s + 1): what `UnifiedVoice.inference_speech_stream` returns for the first batch."""
    _UNIT, _BUSY, _PER = "row", "generating", "row"

    @_session_init
    def __init__(self, model: "UnifiedVoice", inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int, do_sample=False,
                 top_p=1.0, top_k=50, temperature=1.0, repetition_penalty=1.0, length_penalty=1.0, seed: Optional[int] = None,
                 typical_mass: float = 0.0, row_max_new: Optional[Sequence[int]] = None, uniforms=None,
                 row_sampling: Optional[Sequence[dict]] = None, token_scores: bool = False, alignment_heads=None, text_spans=None,
                 alignment_text_cap: Optional[int] = None, code_prefix=None, code_prefix_lens: Optional[Sequence[int]] = None,
                 prefix_chunk: int = 128, prefix_pos_offset: Optional[int] = None, row_filters: Optional[Sequence[Optional[dict]]] = None,
                 **unused):
        """row_filters: per-slot logits filters (`generate`'s engine extension; an entry's missing keys = the session's own filter kwargs):
        the table stays installed for the session and `admit(..., row_filters=)` writes the entries of the slots it refills.
        code_prefix / code_prefix_lens / prefix_chunk: the first batch's code prefixes (`generate`'s engine extension): a row with k given
        codes starts at own step k -- `codes(slot)` returns the full row, prefix included; `admit(..., code_prefix=)` passes the prefixes of
        the utterances it places.  `model.last_prefix` is set by the first `run` and by every such admission.
        alignment_heads / text_spans: the text-attention export (`generate`'s engine extension): the arrays stay installed for the session,
        `admit(..., text_spans=)` passes the spans of the utterances it places (an admission clears the rows of the slots it refills),
        `alignment(slot)` reads the utterance's attention next to `codes(slot)`.  alignment_text_cap: the widest span the session will
        see (default: the first batch's; a multiple of 4 is taken).
        token_scores: per-token log-probabilities (`generate`'s engine extension): the arrays stay installed for the session, an admission
        clears the rows of the slots it refills, `scores(slot)` reads the utterance's scores next to `codes(slot)`.
        row_max_new: per-utterance caps on generated tokens (`generate`'s engine extension): the utterance in a slot emits the stop token from
        its own token index row_max_new[b] on; `admit(..., row_max_new=)` passes the caps of the utterances it places.
        row_sampling: per-slot sampling settings (`generate`'s engine extension; missing keys = the session's scalars, `stream` = the slot):
        the table stays installed for the session and `admit(..., row_sampling=)` rewrites the entries of the slots it refills."""
        model._check_idle("DecodeSession")
        if unused.get("num_beams", 1) != 1:
            if row_sampling is not None:
                raise NotImplementedError("DecodeSession: row_sampling is implemented for num_beams = 1 only")
            raise NotImplementedError("DecodeSession: num_beams = 1 only")
        self._check_kwargs(uniforms, unused)
        align = model._alignment_request(alignment_heads, text_spans, inputs_embeds, "DecodeSession")
        filt = model._filters_for(unused, row_filters, unused.get("group_filters"), inputs_embeds, max_new_tokens, 1, "DecodeSession", row_max_new)
        gp = _gen_params(model.kv_cache, max_new_tokens, model._seed(seed, do_sample, None), do_sample, 1, top_p, top_k, temperature,
                         repetition_penalty, length_penalty, typical_mass)
        self._prefix0 = None                         # the first batch's checked code prefix: installed around the first run()
        if code_prefix is not None or code_prefix_lens is not None:
            nB = int(inputs_embeds.shape[0])
            self._prefix0 = model._code_prefix(code_prefix, code_prefix_lens, nB, model._prefix_caps(max_new_tokens, row_max_new, nB), "DecodeSession")
        self._prefix_args = (int(prefix_chunk), prefix_pos_offset)
        model.last_prefix = None
        self._open(model, inputs_embeds, attention_mask, max_new_tokens, 1, gp)
        if self._prefix0 is not None:
            self.step0 = [-int(k) for k in self._prefix0[1]]     # a row with k given codes has taken k own steps before the session's step 0
        self._given = [0] * self.B if self._prefix0 is None else [int(k) for k in self._prefix0[1]]      # given codes of the utterance in each slot
        B, L = self.B, _lib.lib()
        self._ws = model._workspace(L.itts_gpt_workspace_bytes(model._h, B, self.S, self.S + self.max_new))
        self._codes = model._persistent("codes", (B, self.max_new), torch.int64)
        self._caps = [self.max_new] * B              # host mirror of the slots' caps (what `scores` tells a forced stop token by)
        self._lim = None                             # the installed row-limit table, or None
        if row_max_new is not None:
            self._lim = self._own.row_limits(row_max_new, B)
            self._caps = [int(v) for v in row_max_new]
        self._tab = self._own.sampling("row", None if row_sampling is None else row_sampling_entries(row_sampling, B, _gp_defaults(gp)))
        self._sc = self._own.scores(token_scores, B, self.max_new)      # the installed token-score arrays (logp_model, logp_sampled), or None
        cap = None if align is None or alignment_text_cap is None else max(_alignment_text_cap(align[1]), (int(alignment_text_cap) + 3) // 4 * 4)
        self._al = self._own.alignment(align, B, self.max_new, cap)     # the installed alignment export (span, out), or None
        if align is not None:
            self._text_lens = [l for _, l in align[1]]
        self._open_filters(filt, unused)

    def run(self, n_tokens: int, return_when_finished: int = 0) -> int:
        """advance the batch by up to n_tokens steps; returns the session's step count (stops early when every row has finished -- or, with
        return_when_finished = k > 0, at the engine's next flag check (every 8 steps) once k slots hold a finished utterance, counting the ones
        that were finished before the call: the caller refills slots without polling in short chunks)"""
        limit = self._next_limit(n_tokens, return_when_finished)
        n = C.c_int32(0)
        ingest = self._first and self._prefix0 is not None
        with _HandleState(self.m) as call:           # the prefix is consumed by the first chunk call only: an admission brings its own table
            call.prefix(self._prefix0 if ingest else None, *self._prefix_args)
            rc = _lib.lib().itts_gpt_generate_chunk(
                self.m._h, _lib.ptr(self._x) if self._first else None, _lib.ptr(self._pad), self.B, self.S, C.byref(self._gp), self._pen, 2, None,
                _lib.ptr(self._codes), limit, C.byref(n), _lib.ptr(self._ws), self._ws.numel(), int(self.m.use_graph), _lib.stream_ptr(self.dev))
        _lib.check(rc, "itts_gpt_generate_chunk")
        if ingest:
            self.m._record_prefix(self._prefix0[1], int(n.value) - 1)
        self._first = False
        self.steps = int(n.value)
        return self.steps

    def _own_steps(self, slot: int) -> int:
        """tokens the utterance in `slot` has produced so far (its code columns 0 .. that - 1)"""
        return max(0, min(self.max_new, self.steps - self.step0[slot]))

    def codes(self, slot: int) -> torch.Tensor:
        """the codes of the utterance in `slot` so far (up to, not including, its stop token)"""
        row = self._codes[slot, :self._own_steps(slot)]
        stop = (row == self.m.stop_mel_token).nonzero()
        return row[: int(stop[0])].clone() if stop.numel() else row.clone()

    def scores(self, slot: int) -> "TokenScores":
        """the token scores of the utterance in `slot` so far (one row; its own columns 0 .. own steps - 1, forced columns hold 0.0); the session
        must have been opened with token_scores=True.  A row ended through `stop_row` counts as having run into its cap."""
        if self._sc is None:
            raise RuntimeError("DecodeSession.scores: the session was opened without token_scores=True")
        own = self._own_steps(slot)
        lengths, ended = TokenScores.lengths_of(self._codes[slot:slot + 1, :own], [self._caps[slot]], self.m.stop_mel_token)
        return TokenScores(self._sc[0][slot:slot + 1, :own].clone(), self._sc[1][slot:slot + 1, :own].clone(), lengths, ended,
                           [self._given[slot]] if self._given[slot] else None)

    def alignment(self, slot: int) -> "TokenAlignment":
        """the text attention of the utterance in `slot` so far (one row; its own code columns 0 .. own steps - 1, row 0 and forced columns
        zero); the session must have been opened with alignment_heads"""
        if self._al is None:
            raise RuntimeError("DecodeSession.alignment: the session was opened without alignment_heads")
        own = self._own_steps(slot)
        lengths, _ = TokenScores.lengths_of(self._codes[slot:slot + 1, :own], [self._caps[slot]], self.m.stop_mel_token)
        return TokenAlignment(self._al[1][slot:slot + 1, :own].clone(), [self._text_lens[slot]], lengths)

    def _poll(self) -> List[tuple]:
        """[(number of codes before a stop token so far, finished)] of EVERY slot, from one device reduction and one host synchronisation;
        finished: the utterance has emitted its stop token or used up its max_new_tokens"""
        if self.steps < 1:
            return [(0, False)] * self.B
        own = torch.as_tensor([self.steps - self.step0[b] for b in range(self.B)], device=self.dev)
        cols = torch.arange(self.max_new, device=self.dev)[None, :]
        stop = (self._codes == self.m.stop_mel_token) & (cols < own[:, None])
        first = torch.where(stop.any(dim=1), stop.to(torch.int32).argmax(dim=1), own.clamp(max=self.max_new))       # first stop column, else all own columns
        fin = stop.any(dim=1) | (own > self.max_new)      # (past its last column the engine has the row as stopped: the sampler emits the stop token there)
        host = torch.stack([fin.to(torch.int64), first.to(torch.int64)]).tolist()
        return [(int(host[1][b]), bool(host[0][b])) for b in range(self.B)]

    def finished(self) -> List[int]:
        """slots whose utterance has emitted its stop token or used up its max_new_tokens (one poll: one host synchronisation)"""
        return [b for b, (_, fin) in enumerate(self._poll()) if fin]

    def finished_lengths(self) -> List[tuple]:
        """[(slot, number of codes before its stop token)] of the slots `finished()` reports -- from one poll (the scheduler's:
        `finished()` + `codes()` per slot would synchronise once per slot)"""
        return [(b, n) for b, (n, fin) in enumerate(self._poll()) if fin]

    def progress(self) -> List[tuple]:
        """[(number of codes before a stop token so far, finished)] of EVERY slot, from one poll (a streaming scheduler's: it renders chunks
        of rows that are still generating)"""
        return self._poll()

    def stop_row(self, slot: int) -> None:
        """end the utterance in `slot` at the engine's next step: its entry of the row-limit table becomes 0, written in stream order (the
        sampler emits the stop token from a row's limit on); the session must have been opened with caps, so that the table exists"""
        if self._lim is None:
            raise RuntimeError("DecodeSession.stop_row: the session was opened without row_max_new (there is no row-limit table)")
        if not 0 <= int(slot) < self.B:
            raise ValueError(f"DecodeSession.stop_row: slot {slot} is out of range")
        self._lim[int(slot)] = 0

    def admit(self, slots: Sequence[int], inputs_embeds: torch.Tensor, attention_mask: torch.Tensor,
              row_max_new: Optional[Sequence[int]] = None, row_sampling: Optional[Sequence[dict]] = None, text_spans=None,
              code_prefix=None, code_prefix_lens: Optional[Sequence[int]] = None,
              row_filters: Optional[Sequence[Optional[dict]]] = None) -> None:
        """put new utterances into finished slots: inputs_embeds (n, s', D) / attention_mask (n, s' + 1) as for the first batch, s' <= the first
        batch's s (a cache row holds that prompt + max_new_tokens); row_filters: the new utterances' filter entries (a session opened with
        `row_filters=` only; default: the session's own filter kwargs); row_sampling: the new utterances' sampling settings, given exactly when
        the session was opened with a table; text_spans: their alignment spans, given exactly when it was opened with alignment_heads;
        code_prefix / code_prefix_lens: their code prefixes (as in `generate`, one entry per admitted utterance): an utterance with k given
        codes joins at own step k, `codes(slot)` returns its full row"""
        L = _lib.lib()
        prefix = None
        if code_prefix is not None or code_prefix_lens is not None:
            nn = int(inputs_embeds.shape[0])
            prefix = self.m._code_prefix(code_prefix, code_prefix_lens, nn, self.m._prefix_caps(self.max_new, row_max_new, nn, "admitted row"),
                                         "DecodeSession.admit")
            kmax = max(prefix[1])
        if (text_spans is not None) != (self._al is not None):
            raise ValueError("DecodeSession.admit: text_spans must be given exactly when the session was opened with alignment_heads")
        if text_spans is not None:
            text_spans = alignment_spans(text_spans, int(inputs_embeds.shape[0]), "DecodeSession.admit")
            cap = int(self._al[1].shape[3])
            if any(l > cap for _, l in text_spans):
                raise ValueError(f"DecodeSession.admit: a text span is longer than the session's alignment rows ({cap}); open the session with "
                                 "alignment_text_cap=")
        x, pad, S_new, sl_c, sl = self._admit_inputs(slots, inputs_embeds, attention_mask, row_max_new, row_sampling, self._lim is not None,
                                                     L.itts_gpt_admit_workspace_bytes if prefix is None else
                                                     (lambda h, n_, s_: L.itts_gpt_admit_prefix_workspace_bytes(h, n_, s_, kmax)),
                                                     rewrites=text_spans is not None)
        n = len(sl)
        self._admit_filters(sl, row_filters, int(inputs_embeds.shape[1]) + 1, row_max_new, 1)
        if row_sampling is not None:
            self._rewrite_entries(sl, row_sampling, row_sampling_entries, _gp_defaults(self._gp))
        if text_spans is not None:                   # read every step, like the sampling table: rewritten in stream order (the slots are finished:
            spans = torch.as_tensor(text_spans, dtype=torch.int32).reshape(n, 2)      # the kernel skips them until the admission clears their flag)
            self._al[0][torch.as_tensor(sl, device=self.dev)] = spans.to(self.dev)
        lim = None if row_max_new is None else (C.c_int32 * n)(*[int(v) for v in row_max_new])     # written to the live limits by the engine,
        with _HandleState(self.m) as call:                                                         # after its checks
            call.prefix(prefix, *self._prefix_args)
            rc = L.itts_gpt_admit_rows(self.m._h, _lib.ptr(x), _lib.ptr(pad), sl_c, n, S_new, lim, C.byref(self._gp), self._pen, 2, None,
                                       _lib.ptr(self._codes), _lib.ptr(self._ws), self._ws.numel(), _lib.ptr(self._adm_ws), self._adm_ws.numel(),
                                       _lib.stream_ptr(self.dev))
        _lib.check(rc, "itts_gpt_admit_rows")
        if prefix is not None:
            self.m._record_prefix(prefix[1], 0)
        for i, v in enumerate(sl):
            self._given[v] = 0 if prefix is None else int(prefix[1][i])
            self.step0[v] = self.steps - 1 - self._given[v]
            self._caps[v] = self.max_new if row_max_new is None else int(row_max_new[i])
            if text_spans is not None:
                self._text_lens[v] = text_spans[i][1]


class BeamDecodeSession(_SessionBase):
    """`DecodeSession` for beam search / beam-sample: the slot is a beam GROUP (one utterance's `num_beams` adjacent rows).  `run(n)` advances
    the search by n steps (`itts_gpt_generate_beam_chunk`), `finished()` reports the groups that are done or have reached their cap,
    `result(slot)` finalises one group on the host (`finalize_beam_group`: the ids of its best hypothesis), `admit(slots, ...)` prefills new
    prompts into finished groups (`itts_gpt_admit_beam_groups`) while the others keep searching.  Every group runs on its OWN step and its rows
    on their OWN cache positions, so an admitted utterance ends, bit for bit, with the ids it gets in the same slot of a batch decoded from
    step 0, whatever step it joins at; only a GROUP is bounded by `max_new_tokens`, not the session.  Sampling uses the seeded device stream
    keyed by (seed, own step, slot).

    inputs_embeds (B, s, D) / attention_mask (B, s + 1): one row per utterance, as for `generate`."""
    _UNIT, _BUSY, _PER = "utterance", "searching", "group"

    @_session_init
    def __init__(self, model: "UnifiedVoice", inputs_embeds: torch.Tensor, attention_mask: torch.Tensor, max_new_tokens: int, num_beams: int = 3,
                 do_sample=False, top_p=1.0, top_k=50, temperature=1.0, repetition_penalty=1.0, length_penalty=1.0, seed: Optional[int] = None,
                 typical_mass: float = 0.0, row_max_new: Optional[Sequence[int]] = None, uniforms=None,
                 group_sampling: Optional[Sequence[dict]] = None, group_filters: Optional[Sequence[Optional[dict]]] = None, **unused):
        """group_filters: per-group logits filters (`generate`'s engine extension; an entry's missing keys = the session's own filter kwargs):
        the table stays installed for the session and `admit(..., group_filters=)` writes the entries of the groups it refills.
        row_max_new: per-utterance caps on the search's steps (what `max_new_tokens` is to an utterance decoded alone).
        group_sampling: per-group sampling settings (`generate`'s engine extension; missing keys = the session's scalars, `stream` = the slot):
        the table stays installed for the session and `admit(..., group_sampling=)` rewrites the entries of the groups it refills."""
        model._check_idle("BeamDecodeSession")
        if unused.get("token_scores"):
            raise ValueError("BeamDecodeSession: token_scores=True is implemented for num_beams = 1 only (DecodeSession)")
        if unused.get("alignment_heads") is not None:
            raise ValueError("BeamDecodeSession: alignment_heads is implemented for num_beams = 1 only (DecodeSession)")
        nb = int(num_beams)
        if nb < 2 or nb > 4:
            raise ValueError(f"BeamDecodeSession: num_beams must be 2..4, got {num_beams} (DecodeSession serves num_beams = 1)")
        self._check_kwargs(uniforms, unused)
        filt = model._filters_for(unused, unused.get("row_filters"), group_filters, inputs_embeds, max_new_tokens, nb, "BeamDecodeSession", row_max_new)
        B = inputs_embeds.shape[0]
        if row_max_new is not None and len(row_max_new) != B:
            raise ValueError(f"row_max_new must have one entry per utterance ({B}), got {len(row_max_new)}")
        gp = _gen_params(model.kv_cache, max_new_tokens, model._seed(seed, _any_group_samples(do_sample, group_sampling), None), do_sample, nb,
                         top_p, top_k, temperature, repetition_penalty, length_penalty, typical_mass)
        self._open(model, inputs_embeds, attention_mask, max_new_tokens, nb, gp)
        self.nb, self.length_penalty = nb, float(length_penalty)
        entries = None if group_sampling is None else group_sampling_entries(group_sampling, B, _gp_group_defaults(gp))
        self.slot_length_penalty = [float(length_penalty)] * B if entries is None else [float(e.length_penalty) for e in entries]
        self._ws = model._workspace(_lib.lib().itts_gpt_beam_workspace_bytes(model._h, B, nb, self.S, self.S + self.max_new))
        self._hist_tok, self._hist_par, self._scores, self._hyps, self._n_hyps, self._done = model._beam_state(B, nb, self.max_new)
        self.cap = [self.max_new] * B if row_max_new is None else [max(1, min(self.max_new, int(v))) for v in row_max_new]
        self._host = None                            # host copies of the search state as of the last run()
        self._fresh = set()                          # slots admitted since the last run(): the caller buffers still hold the previous occupant's state
        self._tab = self._own.sampling("group", entries)
        self._open_filters(filt, unused)

    def run(self, n_steps: int, return_when_finished: int = 0) -> int:
        """advance the search by up to n_steps steps; returns the session's step count (stops early when every group has finished -- or, with
        return_when_finished = k > 0, at the engine's next flag check (every 4 steps) once k groups have, counting the ones that had finished
        before the call)"""
        limit = self._next_limit(n_steps, return_when_finished)
        n = C.c_int32(0)
        caps = (C.c_int32 * self.B)(*self.cap) if self._first else None
        _lib.check(_lib.lib().itts_gpt_generate_beam_chunk(
            self.m._h, _lib.ptr(self._x) if self._first else None, _lib.ptr(self._pad), self.B, self.nb, self.S, C.byref(self._gp), self._pen, 2,
            caps, _lib.ptr(self._hist_tok), _lib.ptr(self._hist_par), _lib.ptr(self._scores), _lib.ptr(self._hyps), _lib.ptr(self._n_hyps),
            _lib.ptr(self._done), limit, C.byref(n), _lib.ptr(self._ws), self._ws.numel(), int(self.m.use_graph), _lib.stream_ptr(self.dev)),
            "itts_gpt_generate_beam_chunk")
        self._first = False
        self.steps = int(n.value)
        self._host = None
        self._fresh.clear()
        return self.steps

    def _own_steps(self, slot: int) -> int:
        """beam steps the utterance in `slot` has run so far (at most its cap)"""
        return max(0, min(self.cap[slot], self.steps - self.step0[slot]))

    def _state(self):
        if self._host is None:          # one synchronising copy per poll
            self._host = (self._hist_tok.cpu().numpy(), self._hist_par.cpu().numpy(), self._scores.cpu().numpy(), self._hyps.cpu().numpy(),
                          self._n_hyps.cpu().numpy(), self._done.cpu().numpy())
        return self._host

    def _check_copied_out(self, slot: int, who: str):
        if int(slot) in self._fresh:
            raise RuntimeError(f"BeamDecodeSession.{who}: slot {slot} was admitted since the last run(); its search state is copied out by the next run()")

    def done(self, slot: int) -> bool:
        """the scorer has closed the group (as opposed to: it ran into its cap)"""
        self._check_copied_out(slot, "done")
        return bool(self._state()[5][slot])

    def finished(self) -> List[int]:
        """slots whose group is done or has used up its cap: their result is final and they can be refilled"""
        if self.steps < 1:
            return []
        dn = self._state()[5]
        return [b for b in range(self.B) if b not in self._fresh and (dn[b] or self.steps - self.step0[b] >= self.cap[b])]

    def result(self, slot: int) -> torch.Tensor:
        """ids of the best hypothesis of the utterance in `slot` (without a stop token) -- final once the slot is in `finished()`"""
        self._check_copied_out(slot, "result")
        ht, hp, bs, hy, nh, dn = self._state()
        ids = finalize_beam_group(ht, hp, bs, hy, nh, dn, self._own_steps(slot), self.slot_length_penalty[slot], group=slot, num_beams=self.nb)
        return torch.tensor(ids, dtype=torch.int64, device=self.dev)

    def admit(self, slots: Sequence[int], inputs_embeds: torch.Tensor, attention_mask: torch.Tensor,
              row_max_new: Optional[Sequence[int]] = None, group_sampling: Optional[Sequence[dict]] = None,
              group_filters: Optional[Sequence[Optional[dict]]] = None) -> None:
        """put new utterances into finished groups: inputs_embeds (n, s', D) / attention_mask (n, s' + 1) as for the first batch, s' <= the
        first batch's s (a cache row holds that prompt + max_new_tokens); row_max_new: their caps (default max_new_tokens); group_sampling: the
        new utterances' settings, given exactly when the session was opened with a table; group_filters: their filter entries (a session
        opened with `group_filters=` only; default: the session's own filter kwargs)"""
        L = _lib.lib()
        x, pad, S_new, sl_c, sl = self._admit_inputs(slots, inputs_embeds, attention_mask, row_max_new, group_sampling, None,
                                                     L.itts_gpt_admit_beam_workspace_bytes)
        n = len(sl)
        caps = [self.max_new] * n if row_max_new is None else [max(1, min(self.max_new, int(v))) for v in row_max_new]
        new_entries = None
        self._admit_filters(sl, group_filters, int(inputs_embeds.shape[1]) + 1, caps, self.nb)
        if group_sampling is not None:
            new_entries = self._rewrite_entries(sl, group_sampling, group_sampling_entries, _gp_group_defaults(self._gp))
        _lib.check(L.itts_gpt_admit_beam_groups(self.m._h, _lib.ptr(x), _lib.ptr(pad), sl_c, n, S_new, (C.c_int32 * n)(*caps), C.byref(self._gp),
                                                self._pen, 2, _lib.ptr(self._ws), self._ws.numel(), _lib.ptr(self._adm_ws), self._adm_ws.numel(),
                                                _lib.stream_ptr(self.dev)), "itts_gpt_admit_beam_groups")
        for v, c in zip(sl, caps):
            self.step0[v], self.cap[v] = self.steps - 1, c
        if new_entries is not None:
            for v, e in zip(sl, new_entries):
                self.slot_length_penalty[v] = float(e.length_penalty)
        self._done[sl] = 0                            # the engine has re-opened these groups; the rest of their state is copied out by the next run():
        self._fresh.update(sl)                        # until then result() / done() refuse these slots and finished() leaves them out
        self._host = None


class LatentSession:
    """The teacher-forced latent pass of `UnifiedVoice.forward` (model_v2.py:596-646) as a KV-cached session: the prefix `conds | [start_text,
    ids, stop_text]` is prefilled once, `append(codes_new)` runs only the new mel positions and returns their latents (`itts_gpt_latent_*`).
    The pass is causal and unmasked, so the latents of a code prefix are exactly those the finished utterance has at these positions.  Rows
    keep their own prefix length.  The session owns its workspace tensor and touches nothing of a suspended decode loop: it is not subject
    to `_check_idle`."""

    def __init__(self, model: "UnifiedVoice", conds: torch.Tensor, text_inputs: torch.Tensor, text_lengths: torch.Tensor, max_codes: int,
                 max_append: int):
        if not model._loaded:
            raise RuntimeError("UnifiedVoice: load_state_dict() first")
        self.m, self.dev = model, model.device
        tl = [int(v) for v in torch.as_tensor(text_lengths).reshape(-1).tolist()]
        B, n_cond = int(text_inputs.shape[0]), int(conds.shape[1])
        if len(tl) != B or conds.shape[0] != B:
            raise ValueError(f"latent_session: {B} text rows, {len(tl)} lengths, {conds.shape[0]} conditioning rows")
        if min(tl) < 0 or max(tl) > int(text_inputs.shape[1]):
            raise ValueError(f"latent_session: text_lengths {tl} outside 0 .. {int(text_inputs.shape[1])}")
        # the shared builder pads every row with stop_text ids from its length on: row b's prefix is its first n_cond + tl[b] + 2 positions
        # ([start, ids, ONE stop]); what follows is right padding the engine never reads
        L = max(tl)
        x = model._latent_prefix(conds, text_inputs[:, :L], torch.as_tensor(tl)).contiguous()
        self.prefix_lens = [n_cond + t + 2 for t in tl]
        self.B, self.D = B, int(x.shape[2])
        self.max_prefix, self.max_codes, self.max_append = int(x.shape[1]), int(max_codes), int(max_append)
        Lb = _lib.lib()
        need = Lb.itts_gpt_latent_workspace_bytes(model._h, B, self.max_prefix, self.max_codes, self.max_append)
        if need == 0:
            raise ValueError(f"latent_session: bad shape (rows {B}, prefix {self.max_prefix}, max_codes {max_codes}, max_append {max_append})")
        self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)         # the session's own: NOT the engine's shared workspace
        self._s = C.c_void_p()
        lens = (C.c_int32 * B)(*self.prefix_lens)
        _lib.check(Lb.itts_gpt_latent_open(model._h, _lib.ptr(x), lens, B, self.max_prefix, self.max_codes, self.max_append, _lib.ptr(self._ws),
                                           self._ws.numel(), _lib.stream_ptr(self.dev), C.byref(self._s)), "itts_gpt_latent_open")
        self.appended = 0

    def append(self, codes_new: torch.Tensor) -> torch.Tensor:
        """codes_new (B, n): the next n codes of every row (ended rows: their stop-token padding) -> latents (B, n, D) f32 of those codes' mel
        positions: out[:, i] is the latent `forward` returns at position `appended + i`."""
        if self._s is None or not self._s.value:
            raise RuntimeError("LatentSession.append: the session is closed")
        codes = codes_new.to(self.dev, torch.int64).contiguous()
        if codes.ndim != 2 or codes.shape[0] != self.B:
            raise ValueError(f"LatentSession.append: codes must be ({self.B}, n), got {tuple(codes.shape)}")
        n = int(codes.shape[1])
        out = torch.empty(self.B, n, self.D, dtype=torch.float32, device=self.dev)
        if n == 0:
            return out
        _lib.check(_lib.lib().itts_gpt_latent_append(self._s, _lib.ptr(codes), n, _lib.ptr(out), _lib.stream_ptr(self.dev)),
                   "itts_gpt_latent_append")
        self.appended += n
        return out

    def close(self):
        if self._s is not None and self._s.value:
            _lib.lib().itts_gpt_latent_close(self._s)
        self._s, self._ws = None, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class UnifiedVoiceV1(UnifiedVoice):
    """IndexTTS-1 / 1.5 `UnifiedVoice` (indextts/gpt/model.py): the same GPT-2 stack and generate loop; conditioning is a
    (b,32,D) latent from the Conformer+Perceiver encoder (`get_conditioning`, model.py:495-524), which stays on PyTorch:
    set `conditioning_fn` (e.g. the reference module's bound `get_conditioning`) or pass `conds_latent=`.
    No language embedding, `inference_speech` returns the codes only (model.py:660-716)."""
    _ALLOW_ENCODER_CONDITIONING = True
    _HOST_TENSORS = ("mel_embedding.weight", "mel_pos_embedding.emb.weight", "text_embedding.weight",
                     "text_pos_embedding.emb.weight")
    _OPTIONAL_HOST_TENSORS = ()

    def __init__(self, *args, condition_type="conformer_perceiver", conditioning_fn=None, **kw):
        kw.setdefault("spk_cond_mode", "encoder")
        super().__init__(*args, condition_type=condition_type, **kw)
        self.condition_type = condition_type
        self.conditioning_fn = conditioning_fn

    def get_conditioning(self, speech_conditioning_input, cond_mel_lengths=None):
        if self.conditioning_fn is None:
            raise NotImplementedError("v1 conditioning encoder (Conformer + Perceiver) is outside the engine: set "
                                      "UnifiedVoiceV1.conditioning_fn or pass conds_latent=")
        return self.conditioning_fn(speech_conditioning_input, cond_mel_lengths)

    def prepare_gpt_inputs(self, conditional_latents, text_inputs):                      # model.py:597-659
        return super().prepare_gpt_inputs(conditional_latents, text_inputs, None)

    def inference_speech(self, speech_conditioning_mel, text_inputs, cond_mel_lengths=None, input_tokens=None,
                         num_return_sequences=1, max_generate_length=None, typical_sampling=False, typical_mass=.9,
                         conds_latent=None, uniforms=None, **hf_generate_kwargs):
        if input_tokens is not None or num_return_sequences != 1:
            raise NotImplementedError("input_tokens / num_return_sequences > 1 are not used by the v1 pipeline")
        if typical_sampling and not (typical_mass > 0.0 and typical_mass < 1.0):
            raise ValueError(f"`typical_mass` has to be a float > 0 and < 1, but is {typical_mass}")
        if conds_latent is None:
            if speech_conditioning_mel.ndim == 2:
                speech_conditioning_mel = speech_conditioning_mel.unsqueeze(0)
            if cond_mel_lengths is None:
                cond_mel_lengths = torch.tensor([speech_conditioning_mel.shape[-1]], device=speech_conditioning_mel.device)
            conds_latent = self.get_conditioning(speech_conditioning_mel, cond_mel_lengths)
        input_ids, inputs_embeds, attention_mask = self.prepare_gpt_inputs(conds_latent, text_inputs)
        max_new = (self.max_mel_tokens - 1) if max_generate_length is None else int(max_generate_length)
        hf = dict(hf_generate_kwargs)
        _reject_logits_processor(hf)
        return self.generate(inputs_embeds, attention_mask, max_new, uniforms=uniforms,
                             typical_mass=float(typical_mass) if typical_sampling else 0.0, **hf)

    def forward(self, speech_conditioning_latent, text_inputs, text_lengths, mel_codes, wav_lengths, cond_mel_lengths=None,
                types=None, text_first=True, raw_mels=None, return_attentions=False, return_latent=False,
                clip_inputs=False, conds_latent=None):
        """model.py:526-590 with `return_latent=True` (the only use on the inference path, infer.py:449-454,638-643)."""
        if not return_latent or not text_first or raw_mels is not None or return_attentions or clip_inputs:
            raise NotImplementedError("only the return_latent=True, text_first inference form is on the engine path")
        if conds_latent is None:
            conds_latent = self.get_conditioning(speech_conditioning_latent, cond_mel_lengths)
        if types is not None:
            text_inputs = text_inputs * (1 + types).unsqueeze(-1)
        wl = torch.as_tensor(wav_lengths)
        mel_codes_lengths = torch.ceil(wl / self.mel_length_compression).long() + 1              # model.py:557
        b = text_inputs.shape[0]
        conds = conds_latent.expand(b, -1, -1) if conds_latent.shape[0] == 1 and b > 1 else conds_latent
        return self.forward_latent(conds, text_inputs, torch.as_tensor(text_lengths), mel_codes, mel_codes_lengths)

    __call__ = forward


def pack_gemm_weight(w_kn: torch.Tensor, precision: int, transposed: bool = False) -> torch.Tensor:
    w = w_kn.detach().to("cpu", torch.float32).contiguous()
    K, N = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
    L = _lib.lib()
    out = torch.empty(L.itts_packed_gemm_bytes(K, N, precision), dtype=torch.uint8)
    _lib.check(L.itts_pack_gemm_weight(_lib.ptr(w), K, N, int(transposed), precision, _lib.ptr(out)), "itts_pack_gemm_weight")
    return out


def gemm(a: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor], N: int, precision: int,
         prefill_tiles: bool = False) -> torch.Tensor:
    M, K = a.shape
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    with _lib.on_device(a.device):
        _lib.check(_lib.lib().itts_gemm_forward(_lib.ptr(a.contiguous()), _lib.ptr(w_packed), _lib.ptr(bias), _lib.ptr(out),
                                                M, N, K, precision, int(prefill_tiles), 0, _lib.stream_ptr(a.device)),
                   "itts_gemm_forward")
        return out


def linear_f32(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], cache: Optional[dict] = None, key=None) -> torch.Tensor:
    """`F.linear(x, weight, bias)` on the engine's exact-f32 MFMA GEMM (`itts_gemm_forward`, precision 0) -- the small host-side projections of the
    hot path (the flow-matching decoder's per-step conditioning vectors) run on the same hand-written kernels as everything else instead of a
    vendor BLAS call.  `cache` / `key`: a dict OWNED BY THE CALLER'S MODEL and the parameter's name -- the packed weight is kept there, so it lives
    and dies with the model that owns the parameter (no process-wide table keyed by addresses); without a cache the weight is packed per call.
    K not a multiple of 16 (no shape of the shipped models): `F.linear`."""
    N, K = weight.shape
    if K % 16:
        return F.linear(x, weight.to(x.device), None if bias is None else bias.to(x.device))
    packed = cache.get(key) if cache is not None and key is not None else None
    if packed is None or packed.device != x.device:
        packed = pack_gemm_weight(weight, 0, transposed=True).to(x.device)
        if cache is not None and key is not None:
            cache[key] = packed
    lead = x.shape[:-1]
    a = x.reshape(-1, K).to(torch.float32).contiguous()
    out = gemm(a, packed, None if bias is None else bias.to(x.device, torch.float32).contiguous(), N, 0)
    return out.reshape(*lead, N)


def _spk_proj(x: torch.Tensor, w64: torch.Tensor, b64: torch.Tensor) -> torch.Tensor:
    """spk_emb_proj (model_v2.py:754): a (B, 192) x (192, D) projection, once per batch, outside every loop.  Evaluated in float64 on the host and
    rounded once: the result does not depend on any library's summation order.  That matters: the reference-minted `typical_greedy` fixture holds a
    token whose margin is below f32 summation noise of this projection -- the engine's f32 MFMA GEMM (another order than the reference's CPU sgemm)
    flips it, the correctly rounded value keeps it (profiles/r05d/status.txt).  No vendor BLAS call either way.  w64 / b64: the float64 host copies
    `UnifiedVoice._spk_proj_params()` keeps per model (made once, not per call); only the (B, 192) input crosses to the host."""
    y = x.detach().to("cpu", torch.float64) @ w64.t() + b64
    return y.to(torch.float32).to(x.device)


def gemm_ln(x, g, b, w_packed, bias, N: int, partial=None, bias_prev=None, eps=1e-5):
    """The LayerNorm-fused decode GEMM as a unit op (`itts_gemm_ln_forward`): 1-4 rows, bf16-packed weights.  Returns (out (M, N) f32, x' (M, K))."""
    M, K = x.shape
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    x_out = torch.empty_like(x) if partial is not None else None
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().itts_gemm_ln_forward(_lib.ptr(x.contiguous()), _lib.ptr(partial), _lib.ptr(bias_prev), _lib.ptr(g), _lib.ptr(b),
                                                   float(eps), _lib.ptr(w_packed), _lib.ptr(bias), _lib.ptr(out), _lib.ptr(x_out), M, N, K,
                                                   _lib.stream_ptr(x.device)), "itts_gemm_ln_forward")
    return out, x_out


def layernorm(x, g, b, g2=None, b2=None, eps=1e-5):
    rows, D = x.shape
    out = torch.empty_like(x)
    with _lib.on_device(x.device):
        _lib.check(_lib.lib().itts_layernorm_forward(_lib.ptr(x.contiguous()), _lib.ptr(g), _lib.ptr(b), _lib.ptr(g2),
                                                     _lib.ptr(b2), _lib.ptr(out), rows, D, float(eps), _lib.stream_ptr(x.device)),
                   "itts_layernorm_forward")
        return out
