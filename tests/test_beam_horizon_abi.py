"""tfasr_{ctc,rnnt}_beam_commit_horizon and tfasr_{ctc,rnnt}_beam_compact (added under ABI 44): the symbols and every host-side check
answer without a GPU, and so do the Python stream objects' and the session's argument checks."""
import ctypes
import os
import re

import pytest

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import streaming

NEW = {"tfasr_rnnt_beam_commit_horizon": 17, "tfasr_rnnt_beam_compact": 14, "tfasr_ctc_beam_commit_horizon": 15, "tfasr_ctc_beam_compact": 13}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
INVALID = 1
f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch


def test_symbols_declared_and_exported_under_the_same_abi():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    src = open(HEADER).read()
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert "#define TFASR_BEAM_MAX_HORIZON 4096" in src and K.MAX_HORIZON == 4096


def test_ctc_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    B, C, Tcap, V, W = 3, 4, 19, 6, 8
    n = ctypes.c_size_t(0)
    assert lib.tfasr_ctc_beam_stream_workspace_size(B, C, Tcap, V, W, ctypes.byref(n)) == 0
    need = n.value

    def commit(com=f, toks=f, n_=f, hs=f, H=8, width=8, B_=B, W_=W, ws=f, wsb=need):
        return lib.tfasr_ctc_beam_commit_horizon(None, com, toks, n_, hs, H, B_, C, Tcap, V, W_, width, ws, wsb, None)

    for kw in (dict(com=None), dict(toks=None), dict(n_=None), dict(hs=None), dict(H=0), dict(H=-3), dict(H=4097), dict(width=0), dict(B_=0),
               dict(W_=0), dict(W_=65), dict(ws=None), dict(wsb=need - 1)):
        assert commit(**kw) == INVALID, kw

    def compact(mask=f, com=f, hs=f, H=8, out=f, B_=B, W_=W, ws=f, wsb=need):
        return lib.tfasr_ctc_beam_compact(mask, com, hs, H, out, B_, C, Tcap, V, W_, ws, wsb, None)

    # (a compaction names its streams: no mask is a bad mask; a horizon state goes with its horizon, none with 0)
    for kw in (dict(mask=None), dict(com=None), dict(out=None), dict(H=0), dict(H=4097), dict(hs=None, H=8), dict(B_=0), dict(W_=65),
               dict(ws=None), dict(wsb=need - 1)):
        assert compact(**kw) == INVALID, kw


def test_transducer_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    B, Tcap, U, J, V, W = 2, 20, 16, 16, 5, 4
    n = ctypes.c_size_t(0)
    assert lib.tfasr_rnnt_beam_workspace_size(B, Tcap, U, J, V, W, ctypes.byref(n)) == 0
    need = n.value

    def commit(com=f, toks=f, n_=f, hs=f, H=4, width=8, blank=0, B_=B, W_=W, ws=f, wsb=need):
        return lib.tfasr_rnnt_beam_commit_horizon(None, com, toks, n_, hs, H, B_, Tcap, U, J, V, W_, width, blank, ws, wsb, None)

    for kw in (dict(com=None), dict(toks=None), dict(n_=None), dict(hs=None), dict(H=0), dict(H=4097), dict(width=0), dict(blank=V),
               dict(blank=-1), dict(B_=0), dict(W_=65), dict(ws=None), dict(wsb=need - 1)):
        assert commit(**kw) == INVALID, kw

    def compact(mask=f, com=f, hs=f, H=4, out=f, B_=B, W_=W, ws=f, wsb=need):
        return lib.tfasr_rnnt_beam_compact(mask, com, hs, H, out, B_, Tcap, U, J, V, W_, ws, wsb, None)

    for kw in (dict(mask=None), dict(com=None), dict(out=None), dict(H=0), dict(hs=None, H=4), dict(B_=0), dict(W_=0), dict(ws=None),
               dict(wsb=need - 1)):
        assert compact(**kw) == INVALID, kw


def test_python_surface():
    for cls in (K.RnntBeamStream, K.CtcBeamStream):
        assert callable(cls.compact) and callable(cls.commit)
    assert callable(streaming.StreamingRecognizer.compact)
    assert streaming.check_commit_horizon(None, 0) is None and streaming.check_commit_horizon(8, 4) == 8
    with pytest.raises(ValueError, match="beam_width"):
        streaming.check_commit_horizon(8, 0)
    with pytest.raises(ValueError, match="commit_horizon"):
        streaming.check_commit_horizon(0, 4)
    with pytest.raises(ValueError, match="commit_horizon"):
        streaming.check_commit_horizon(4097, 4)
    with pytest.raises(ValueError, match="beam_width"):  # judged before the model is looked at
        streaming.StreamingRecognizer(None, 1, commit_horizon=8)
    with pytest.raises(ValueError, match="commit_horizon"):
        streaming.StreamingRecognizer(None, 1, beam_width=4, commit_horizon=0)
