"""Host side of the device logits filters (itts_gpt_set_logits_filters): the C ABI entry, the one builder behind every decode entry
(`gpt.logits_filters`: HF's "off" rules and its errors) and the fixtures minted by tools/make_golden_gpt_filters.py.  No GPU."""
import ctypes as C
import glob
import json
import os
import re

import numpy as np
import pytest

from indextts_amd import _lib, gpt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, STOP = 8194, 8193
# the cases the fixtures must cover
REQUIRED = ("minnew", "minnew4", "minlen", "ngram2", "ngram3", "suppress", "decay", "sample_minp", "sample_epsilon", "sample_eta", "sample_order",
            "beam_sample", "beam_suppress")


def build(num_beams=1, max_new=28, prompt_len=None, **kw):
    return gpt.logits_filters(kw, V, STOP, max_new, num_beams, "test", prompt_len=prompt_len)


def test_header_declares_the_entry_as_a_v13_addition():
    h = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert "#define ITTS_ABI_VERSION 13" in h
    assert "int itts_gpt_set_logits_filters(itts_gpt* h, const itts_logits_filters* f);" in h
    assert re.search(r"/\* Logits filters \(v13, additive: [^)]*\)", h)
    doc = h[h.index("/* Logits filters (v13, additive"):h.index("int itts_gpt_set_logits_filters")]
    assert "transformers_generation_utils.py:843-1070" in doc and "model_v2.py:815-820" in doc      # the reference lines it replaces
    for field in ("min_new_tokens", "min_length", "no_repeat_ngram_size", "decay_start", "min_p", "epsilon_cutoff", "eta_cutoff", "n_suppress",
                  "n_begin_suppress", "n_decay", "suppress_ids", "begin_suppress_ids", "decay_table"):
        assert re.search(r"\b%s\b" % field, doc), field


def test_signature_and_struct_layout():
    restype, argtypes = _lib.SIGNATURES["itts_gpt_set_logits_filters"]
    assert restype is C.c_int and argtypes == [C.c_void_p, C.POINTER(_lib.LogitsFilters)]
    assert _lib.ABI_VERSION == 13
    assert [n for n, _ in _lib.LogitsFilters._fields_] == [
        "min_new_tokens", "min_length", "no_repeat_ngram_size", "decay_start", "min_p", "epsilon_cutoff", "eta_cutoff", "n_suppress",
        "n_begin_suppress", "n_decay", "suppress_ids", "begin_suppress_ids", "decay_table"]
    assert C.sizeof(_lib.LogitsFilters) == 40 + 3 * C.sizeof(C.c_void_p) and _lib.LogitsFilters.suppress_ids.offset == 40


def test_null_handle_is_an_argument_error():
    L = _lib.lib()
    assert L.itts_gpt_set_logits_filters(None, None) == _lib.ERR_ARG
    assert b"null handle" in L.itts_last_error()
    assert L.itts_gpt_set_logits_filters(None, C.byref(_lib.LogitsFilters())) == _lib.ERR_ARG


def test_values_hf_treats_as_off_install_nothing():
    assert build() is None
    assert build(no_repeat_ngram_size=None, bad_words_ids=None, min_length=None, min_new_tokens=None, suppress_tokens=None,
                 begin_suppress_tokens=None, epsilon_cutoff=None, eta_cutoff=None, exponential_decay_length_penalty=None, min_p=None) is None
    assert build(no_repeat_ngram_size=0, min_length=0, min_new_tokens=0) is None
    assert build(epsilon_cutoff=0.0, eta_cutoff=0.0) is None and build(epsilon_cutoff=1.0, eta_cutoff=1.5) is None
    assert build(min_length=-3) is None                       # `min_length > 0` guards the processor
    assert build(suppress_tokens=[], begin_suppress_tokens=[]) is None
    assert build(bad_words_ids=[[STOP]]) is None              # NoBadWordsLogitsProcessor drops an entry equal to [eos]
    f = build(min_p=0.0)                                      # min_p: whenever not None
    assert f is not None and f.min_p == 0.0 and f.epsilon_cutoff == 0.0 and f.eta_cutoff == 0.0


def test_builder_fills_the_record():
    f = build(min_new_tokens=5, min_length=40, no_repeat_ngram_size=3, suppress_tokens=[3, 4], begin_suppress_tokens=(9,),
              bad_words_ids=[[7], [STOP]], exponential_decay_length_penalty=(2, 1.1), min_p=0.05, epsilon_cutoff=3e-4, eta_cutoff=0.5, max_new=6)
    assert (f.min_new_tokens, f.no_repeat_ngram_size, f.decay_start) == (5, 3, 2)
    assert f.min_length == 0                                  # a given min_new_tokens takes precedence (the reference's generate overwrites min_length)
    assert build(min_length=40).min_length == 40
    assert [f.suppress_ids[i] for i in range(f.n_suppress)] == [7, 3, 4]
    assert [f.begin_suppress_ids[i] for i in range(f.n_begin_suppress)] == [9]
    # HF: torch.abs(scores) * (pow(factor, k) - 1): a Python double handed to an f32 multiply
    want = [0.0, 0.0, 0.0] + [float(np.float32(pow(1.1, k) - 1)) for k in (1, 2, 3)]
    assert f.n_decay == 6 and [f.decay_table[i] for i in range(6)] == want
    assert f.min_p == np.float32(0.05) and f.epsilon_cutoff == np.float32(3e-4) and f.eta_cutoff == 0.5
    assert build(min_new_tokens=5).min_p < 0                  # off


def test_builder_errors():
    with pytest.raises(NotImplementedError, match="multi-token"):
        build(bad_words_ids=[[5], [6, 7]])
    with pytest.raises(NotImplementedError, match="num_beams = 1 only"):
        build(num_beams=3, no_repeat_ngram_size=2)
    assert build(num_beams=3, no_repeat_ngram_size=0, min_new_tokens=2) is not None
    for bad in (dict(min_p=1.5), dict(min_p=-0.1), dict(min_new_tokens=2.5), dict(min_length=7.0), dict(no_repeat_ngram_size=1.5),
                dict(bad_words_ids=[]), dict(bad_words_ids=[3]), dict(bad_words_ids=[[-1]]), dict(bad_words_ids=[[]]),
                dict(suppress_tokens=[V]), dict(begin_suppress_tokens=[-1]), dict(bad_words_ids=[[V]]),
                dict(exponential_decay_length_penalty=(1,)), dict(exponential_decay_length_penalty=(-1, 1.1)),
                dict(exponential_decay_length_penalty=(1.5, 1.1)), dict(exponential_decay_length_penalty=(1, 0.0))):
        with pytest.raises(ValueError):
            build(**bad)
    with pytest.raises(ValueError, match="Unfeasible length constraints"):
        build(min_new_tokens=29, prompt_len=16)
    with pytest.raises(ValueError, match="Unfeasible length constraints"):
        build(min_length=45, prompt_len=16)
    assert build(min_new_tokens=28, prompt_len=16).min_new_tokens == 28


def test_the_ten_kwargs_left_the_unsupported_set_and_the_rest_still_raises():
    assert not set(gpt._LOGITS_FILTER_KWARGS) & gpt._UNSUPPORTED_GENERATE_KWARGS and len(gpt._LOGITS_FILTER_KWARGS) == 10
    for k in ("renormalize_logits", "sequence_bias", "typical_p", "encoder_no_repeat_ngram_size", "forced_eos_token_id", "guidance_scale"):
        assert k in gpt._UNSUPPORTED_GENERATE_KWARGS
    m = gpt.UnifiedVoice.__new__(gpt.UnifiedVoice)            # generate() refuses before it touches the engine
    m._loaded = True
    with pytest.raises(NotImplementedError, match="renormalize_logits") as e:
        m.generate(None, None, 8, renormalize_logits=True, min_new_tokens=3)
    assert "min_new_tokens" in str(e.value).split("supported:")[1]          # ... and names what is accepted
    with pytest.raises(NotImplementedError, match="renormalize_logits"):
        gpt.DecodeSession._check_kwargs(None, dict(renormalize_logits=True))
    # call-wide: a per-row / per-group table entry carrying one of them is still an unknown key
    defaults = dict(do_sample=0, top_k=50, top_p=1.0, temperature=1.0, repetition_penalty=1.0, typical_mass=0.0, seed=0, length_penalty=1.0)
    with pytest.raises(ValueError, match="unknown keys"):
        gpt.row_sampling_entries([dict(min_p=0.1)], 1, defaults)
    with pytest.raises(ValueError, match="unknown keys"):
        gpt.group_sampling_entries([dict(min_new_tokens=3)], 1, defaults)


def test_every_fixture_differs_from_its_plain_run(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "gpt_filters_*.npz")))
    tags = [os.path.basename(f)[len("gpt_filters_"):-len(".npz")] for f in files]
    assert set(REQUIRED) <= set(tags), sorted(set(REQUIRED) - set(tags))
    plain = np.load(os.path.join(golden_dir, "gpt_greedy.npz"))["codes"]
    for f, tag in zip(files, tags):
        z = np.load(f)
        kw = json.loads(str(z["kwargs"]))
        assert kw and set(kw) <= set(gpt._LOGITS_FILTER_KWARGS), (tag, kw)
        a, b = z["codes"], z["codes_plain"]
        assert a.shape != b.shape or not np.array_equal(a, b), f"{tag}: the kwargs change nothing"
        if int(z["gen"][0]):
            assert float(z["margin"]) >= 1e-4, f"{tag}: a draw {float(z['margin']):.2e} from a CDF edge"
        if tag in ("minnew", "minnew4", "minlen"):            # the shapes and weights of gpt_greedy.npz
            assert np.array_equal(b, plain), tag
        assert os.path.getsize(f) < 64 * 1024
