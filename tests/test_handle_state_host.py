"""CPU tests of who owns the state a GPT decode entry installs on the engine handle (`gpt._HandleState`): every entry -- `generate` at
num_beams = 1 and 2, `generate_chunks`, opening a `DecodeSession` / `BeamDecodeSession` -- runs against a recording stand-in for the engine
library that fails its k-th call, for every k; whatever fails, the entry raises, nothing stays installed on the handle and the model is idle.
The shapes are the smallest that reach every install: B = 2 rows, prompt s = 4, D = 8, max_new_tokens = 8, num_beams = 2 on the beam entries.
The success path of the same scope on the engine: tests/test_gpu_gpt.py::test_installed_state_leaves_with_its_call_or_session."""
import ctypes as C

import pytest
import torch

from indextts_amd import _lib, gpt
from tests.test_code_prefix_host import _bare

B, S0, D, MAX_NEW = 2, 4, 8, 8


class _Engine:
    """Stand-in for the engine library.  An `itts_gpt_set_*` call records its state as installed when its first argument after the handle is
    non-NULL / non-zero and as cleared when it is NULL / 0 (a NULL call always clears, as in the engine).  The calls that can refuse -- the
    installing setter calls and the `itts_gpt_generate*` / admission calls -- are counted, and the `fail_at`-th of them returns ERR_ARG; a
    setter that fails has still left its state behind (the worst a setter that fails half-way could do).  The workspace-size entries return
    a small number; a generate call reports that it ran to its step limit."""

    def __init__(self, fail_at=None):
        self.fail_at, self.refusable, self.installed, self.log, self._prefix_max = fail_at, 0, set(), [], 0

    def itts_last_error(self):
        return b"the stand-in was told to fail this call"

    def __getattr__(self, name):
        if not name.startswith("itts_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _refuses(self) -> bool:
        self.refusable += 1
        return self.refusable == self.fail_at

    def _call(self, name, args):
        self.log.append(name)
        if name.startswith("itts_gpt_set_"):
            what = name[len("itts_gpt_set_"):]
            if args[1] is None or (isinstance(args[1], int) and args[1] == 0):
                self.installed.discard(what)
                return 0
            self.installed.add(what)
            if what == "code_prefix":
                self._prefix_max = max(args[2])
            return _lib.ERR_ARG if self._refuses() else 0
        if name.endswith("workspace_bytes"):
            return 64
        if name == "itts_gpt_last_prefix":
            args[1]._obj.value, args[2]._obj.value = self._prefix_max, 1
            return 0
        if name.startswith("itts_gpt_generate") or name.startswith("itts_gpt_admit"):
            if self._refuses():
                return _lib.ERR_ARG
            for i, a in enumerate(args):                     # n_steps_out: the step limit before it, else the whole call
                if isinstance(getattr(a, "_obj", None), C.c_int32):
                    a._obj.value = args[i - 1] if isinstance(args[i - 1], int) else MAX_NEW
        return 0


def _model(monkeypatch, engine):
    m = _bare()
    m._h, m._bufs, m._ws, m.use_graph, m._stream_open = C.c_void_p(), {}, None, True, False      # (a NULL handle: nothing for __del__ to destroy)
    m._emb = {"mel_embedding.weight": torch.zeros(100, D), "mel_pos_embedding.emb.weight": torch.zeros(MAX_NEW + 4, D)}
    m._sync = lambda: None                                   # (the device stream a setter waits for: there is none here)
    m._persistent("codes", (B, MAX_NEW), torch.int64).zero_()          # no row ever holds the stop token: every loop runs to its limit
    zeros = lambda *a: tuple(torch.zeros_like(t) for t in gpt.UnifiedVoice._beam_state(m, *a))
    m._beam_state = zeros                                    # (a search state the host finalisation can walk)
    monkeypatch.setattr(_lib, "lib", lambda: engine)
    monkeypatch.setattr(_lib, "stream_ptr", lambda device=None: None)
    return m


def _inputs():
    return torch.zeros(B, S0, D), torch.ones(B, S0 + 1)


SAMPLING = [{}, dict(do_sample=True, top_k=5, seed=3)]
FILTERS = [None, dict(min_new_tokens=2)]
ROW_EXTRAS = dict(row_sampling=SAMPLING, row_filters=FILTERS, token_scores=True, alignment_heads=[(0, 0), (2, 1)], text_spans=[(1, 2), (0, 3)],
                  code_prefix=[[1, 2], None], prefix_chunk=4)
CAPS = [8, 6]
GROUP_EXTRAS = dict(num_beams=2, group_sampling=SAMPLING, group_filters=FILTERS)

# entry -> (what it runs, the state it must have had installed at some point when nothing fails)
ENTRIES = {
    "generate": (lambda m: m.generate(*_inputs(), MAX_NEW, row_max_new=CAPS, **ROW_EXTRAS),
                 {"row_limits", "row_sampling", "row_filters", "token_scores", "alignment", "code_prefix"}),
    "generate_beam": (lambda m: m.generate(*_inputs(), MAX_NEW, **GROUP_EXTRAS), {"group_sampling", "row_filters"}),
    "generate_beam_capped": (lambda m: m.generate(*_inputs(), MAX_NEW, row_max_new=CAPS, **GROUP_EXTRAS), {"group_sampling", "row_filters"}),
    "generate_chunks": (lambda m: list(m.generate_chunks(*_inputs(), MAX_NEW, 4, 1, **ROW_EXTRAS)),
                        {"row_sampling", "row_filters", "token_scores", "alignment", "code_prefix"}),
    "DecodeSession": (lambda m: gpt.DecodeSession(m, *_inputs(), MAX_NEW, row_max_new=CAPS, **ROW_EXTRAS),
                      {"row_limits", "row_sampling", "row_filters", "token_scores", "alignment"}),
    "BeamDecodeSession": (lambda m: gpt.BeamDecodeSession(m, *_inputs(), MAX_NEW, row_max_new=CAPS, **GROUP_EXTRAS),
                          {"group_sampling", "row_filters"}),
}


def _seen_installed(engine) -> set:
    return {n[len("itts_gpt_set_"):] for n in engine.log if n.startswith("itts_gpt_set_")}


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_whatever_call_fails_nothing_stays_on_the_handle(monkeypatch, entry):
    run, expected = ENTRIES[entry]
    ok = _Engine()
    m = _model(monkeypatch, ok)
    out = run(m)                                             # nothing fails: how many calls could have
    assert expected <= _seen_installed(ok) and ok.refusable >= len(expected) + (0 if "Session" in entry else 1)
    if "Session" in entry:
        assert ok.installed == expected and m._stream_open is True
        out.close()
    assert ok.installed == set() and m._stream_open is False
    for k in range(1, ok.refusable + 1):
        eng = _Engine(fail_at=k)
        m = _model(monkeypatch, eng)
        with pytest.raises(_lib.HipEngineError, match="told to fail"):
            run(m)
        assert eng.refusable >= k, k
        assert eng.installed == set(), (k, eng.log[-6:], eng.installed)
        assert m._stream_open is False, k
        m._check_idle("x")


def _open(monkeypatch, cls):
    eng = _Engine()
    m = _model(monkeypatch, eng)
    return eng, m, ENTRIES[cls.__name__][0](m)


@pytest.mark.parametrize("cls", [gpt.DecodeSession, gpt.BeamDecodeSession])
def test_close_clears_what_the_session_installed_and_may_be_repeated(monkeypatch, cls):
    eng, m, s = _open(monkeypatch, cls)
    assert eng.installed and m._stream_open is True
    with pytest.raises(RuntimeError, match="is open on this engine"):
        m._check_idle("x")
    assert s.run(4, return_when_finished=1) == 4             # sets the early-return threshold (and ingests the first batch's prefix)
    assert "chunk_return" in eng.installed and "code_prefix" not in eng.installed
    assert ("itts_gpt_set_code_prefix" in eng.log) == (cls is gpt.DecodeSession)
    s.close()
    assert eng.installed == set() and m._stream_open is False
    n = len(eng.log)
    s.close()
    assert eng.installed == set() and m._stream_open is False and len(eng.log) == n      # nothing left to clear: no engine call
    with cls(m, *_inputs(), MAX_NEW) as plain:               # a plain session installs nothing; the context manager closes it
        assert eng.installed == set() and plain.run(8) == 8
    assert eng.installed == set() and m._stream_open is False


def test_a_chunk_call_that_fails_takes_its_prefix_along_and_leaves_the_session_to_close(monkeypatch):
    eng, m, s = _open(monkeypatch, gpt.DecodeSession)
    held = set(eng.installed)
    eng.fail_at = eng.refusable + 3                          # the threshold and the prefix install go through, the chunk call is refused
    with pytest.raises(_lib.HipEngineError, match="itts_gpt_generate_chunk"):
        s.run(4, return_when_finished=1)
    assert eng.installed == held | {"chunk_return"}          # the prefix left with its call; the session's own state is the session's
    s.close()
    assert eng.installed == set() and m._stream_open is False


@pytest.mark.parametrize("cls", [gpt.DecodeSession, gpt.BeamDecodeSession])
def test_a_session_that_did_not_open_needs_no_guards(monkeypatch, cls):
    """`close` reads nothing that `__init__` had not set yet: whichever step of `__init__` raised -- an argument check before anything was
    installed, or any install -- closing the half-built object neither raises nor finds anything left to clear"""
    kwargs = dict(row_max_new=CAPS, **(ROW_EXTRAS if cls is gpt.DecodeSession else GROUP_EXTRAS))
    eng = _Engine()
    m = _model(monkeypatch, eng)
    s = object.__new__(cls)
    with pytest.raises(NotImplementedError, match="uniforms"):
        s.__init__(m, *_inputs(), MAX_NEW, uniforms=torch.zeros(MAX_NEW, B))
    s.close()
    assert eng.log == [] and m._stream_open is False
    cls(m, *_inputs(), MAX_NEW, **kwargs).close()
    for k in range(1, eng.refusable + 1):
        eng = _Engine(fail_at=k)
        m = _model(monkeypatch, eng)
        s = object.__new__(cls)
        with pytest.raises(_lib.HipEngineError):
            s.__init__(m, *_inputs(), MAX_NEW, **kwargs)
        n = len(eng.log)
        s.close()
        assert eng.installed == set() and len(eng.log) == n and m._stream_open is False, k


def test_the_owner_clears_in_reverse_and_past_an_undo_that_raises():
    calls = []

    class M:
        def _install_filters(self, f): calls.append(("set filters", f))
        def _uninstall_filters(self, f): calls.append(("clear filters", f))
        def _install_scores(self, b, n): calls.append("set scores"); return "arrays"
        def _uninstall_scores(self): calls.append("clear scores"); raise RuntimeError("undo failed")
        def _install_alignment(self, *a): calls.append("set alignment"); raise ValueError("refused")
        def _uninstall_alignment(self): calls.append("clear alignment")

    with pytest.raises(RuntimeError, match="undo failed"):
        with gpt._HandleState(M()) as own:
            own.filters("f")
            own.filters(None)                                # nothing to install: nothing to clear
            assert own.scores(True, 2, 8) == "arrays" and own.scores(False, 2, 8) is None
            own.alignment(("pairs", "spans"), 2, 8)
    # the undo of the setter that raised half-way is there too, the order is the reverse, and the undo that raised stopped nothing
    assert calls == [("set filters", "f"), "set scores", "set alignment", "clear alignment", "clear scores", ("clear filters", "f")]
