"""The token-selection kernels (`sample_kernel`, `beam_rows_kernel`, `beam_step_kernel`, `beam_apply_kernel`) on the crafted score rows of
tests/select_matrix.py: ids compared EXACTLY with the table's (the oracle's under the engine's tie rule; the two kinds of case the oracle
cannot state are named there), through `inference_speech` -> `generate` on

* the scalar call and the per-row / per-group tables (a case without a table of its own also runs with its scalars as every entry);
* the fp32 engine for every case, the bf16 engine for one case per family (the zero head weight keeps the logits exact there too);
* the step graph on, and off for one case per family;
* both top-k paths (option `sample_radix`) where the case lists them.

With `token_scores=True` every non-beam case also holds `logp_model` to the f64 `log_softmax(row)[token]` and `logp_sampled` to the f64 share
of the kept set (greedy: of the processed row), under the gate of tests/test_gpu_token_scores.py -- which also proves the kernels saw the row.

Every case builds its own tiny engine: a head bias reloaded into a finalised handle lands in a new buffer, which a cached decode graph does not
know about.  tests/test_select_matrix_host.py holds what the table rests on."""
import pytest
import torch

from tests import select_matrix as M
from tests.test_gpu_token_scores import GATE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = M.cases()


# for the bf16 engine and for the loop without the step graph: per family one case on the scalars and one with a table of its own
PER_FAMILY = [M.by_name(n) for n in ("penalty-halves-positive-V8194", "stop-wins-at-step-3-V8194", "topk-edge-8-way-tie-V8194",
                                     "four-setting-sets-one-row-V8194", "beam2-lp2.0-stop-second-V200", "beam3-search-group-table-V8194",
                                     "beam2-sample-group-table-V200")]


def _engine(case, prec="fp32"):
    from indextts_amd import gpt
    cfg = M.config(case.V)
    m = gpt.UnifiedVoice(spk_cond_mode="campplus", layers=cfg.layers, model_dim=cfg.model_dim, heads=cfg.heads, max_text_tokens=cfg.max_text_tokens,
                         max_mel_tokens=cfg.max_mel_tokens, number_text_tokens=cfg.number_text_tokens, number_mel_codes=cfg.number_mel_codes,
                         start_mel_token=cfg.start_mel_token, stop_mel_token=cfg.stop_mel_token, precision=prec, device=DEV)
    m.load_state_dict(M.weights(case.V, case.row))
    m.post_init_gpt2_config(kv_cache=True, half=prec == "bf16")
    return m


_TABLE_KEYS = ("do_sample", "top_k", "top_p", "temperature", "repetition_penalty", "typical_mass", "min_tokens_to_keep", "length_penalty")


def _call(m, case, table: bool, token_scores: bool = False):
    """one `inference_speech` call of the case -> ids on the host.  table: the settings go through `row_sampling` / `group_sampling` (the case's
    own entries, or its scalars as every entry); else through the call's scalars (cases without a table of their own)."""
    st = case.st
    beams = case.family == "beam"
    text, langs, style, emo = M.inputs(case.B)
    mass = float(st.get("typical_mass", 0.0))
    kw = dict(do_sample=bool(st.get("do_sample", False)), num_beams=int(st.get("num_beams", 1)), top_k=int(st.get("top_k", 50)),
              top_p=float(st.get("top_p", 1.0)), temperature=float(st.get("temperature", 1.0)), repetition_penalty=float(st.get("repetition_penalty", 1.0)),
              length_penalty=float(st.get("length_penalty", 1.0)), typical_sampling=mass > 0.0, typical_mass=mass if mass > 0.0 else 0.9)
    if table:
        entries = [{k: v for k, v in e.items() if k in _TABLE_KEYS and (beams or k != "length_penalty")} for e in M.unit_settings(case)]
        kw["group_sampling" if beams else "row_sampling"] = entries
    else:
        assert case.rows is None
    if case.row_max_new is not None:
        kw["row_max_new"] = list(case.row_max_new)
    if token_scores:
        kw["token_scores"] = True
    ids = m.inference_speech(None, text, langs=langs, emo_vec=emo, campplus_embedding=style, max_generate_length=case.max_new, uniforms=case.uniforms,
                             **kw)[0]
    return ids.cpu()


def _check(got, want, what):
    assert got.shape == want.shape and torch.equal(got, want), f"{what}: engine {got.tolist()} expected {want.tolist()}"


def _paths(case):
    return ([False] if case.rows is None else []) + [True]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_ids_fp32(case):
    from indextts_amd import _lib
    want = M.expected_ids(case)
    m = _engine(case)
    try:
        for radix in case.radix:
            if radix is not None:
                _lib.set_option("sample_radix", radix)
            for table in _paths(case):
                what = f"{case.name} [{case.why}] sample_radix={radix} {'table' if table else 'scalars'}"
                got = _call(m, case, table)
                print(f"{what}: {got.tolist()}")
                _check(got, want, what)
                if case.cap or case.name.startswith("beam3-more-ties"):      # more ties than slots: the same survivors in every call
                    _check(_call(m, case, table), want, what + " (second call)")
    finally:
        _lib.set_option("sample_radix", -1)


@pytest.mark.parametrize("case", [c for c in CASES if c.family != "beam"], ids=[c.name for c in CASES if c.family != "beam"])
def test_token_scores_fp32(case):
    """ids unchanged by the flag; logp_model / logp_sampled of every token the selection chose itself against f64, 0.0 in the forced columns"""
    want = M.expected_ids(case)
    ref = []
    ids64 = M.run_rows(case, torch.float64, scores=ref)
    assert ids64.shape == want.shape and torch.equal(ids64, want)
    m = _engine(case)
    got = _call(m, case, case.rows is not None, token_scores=True)
    _check(got, want, case.name)
    ts = m.last_scores
    lm, ls = ts.logp_model.cpu().double(), ts.logp_sampled.cpu().double()
    worst = 0.0
    for b in range(case.B):
        n = min(len(ref[b]), got.shape[1])
        assert int(ts.lengths[b]) == n, (b, int(ts.lengths[b]), n)
        for j in range(n):
            worst = max(worst, abs(float(lm[b, j]) - ref[b][j][0]), abs(float(ls[b, j]) - ref[b][j][1]))
        assert bool((lm[b, n:] == 0).all()) and bool((ls[b, n:] == 0).all()), "a forced column holds a score"
    print(f"{case.name}: max |engine - f64| = {worst:.3e} (gate {GATE:.3e})")
    assert worst <= GATE


@pytest.mark.parametrize("case", PER_FAMILY, ids=[c.name for c in PER_FAMILY])
def test_ids_bf16(case):
    want = M.expected_ids(case)
    m = _engine(case, "bf16")
    for table in _paths(case):
        _check(_call(m, case, table), want, f"{case.name} bf16 {'table' if table else 'scalars'}")


@pytest.mark.parametrize("case", PER_FAMILY, ids=[c.name for c in PER_FAMILY])
def test_ids_without_the_step_graph(case):
    want = M.expected_ids(case)
    m = _engine(case)
    m.use_graph = False
    for table in _paths(case):
        _check(_call(m, case, table), want, f"{case.name} no graph {'table' if table else 'scalars'}")
    assert m.graph_stats()["captures"] == 0, "the loop captured a graph with use_graph off"
