"""The beam searches in pieces (tfasr_rnnt_beam_reset / _advance / _commit / _nbest_states, tfasr_ctc_beam_reset / _advance / _commit /
_nbest; added under ABI 44) and the beam session's arguments: the symbols and every host-side check answer without a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import streaming

NEW = {"tfasr_rnnt_beam_reset": 11, "tfasr_rnnt_beam_advance": 27, "tfasr_rnnt_beam_commit": 15, "tfasr_rnnt_beam_nbest_states": 18,
       "tfasr_ctc_beam_stream_workspace_size": 6, "tfasr_ctc_beam_reset": 9, "tfasr_ctc_beam_advance": 14, "tfasr_ctc_beam_commit": 13,
       "tfasr_ctc_beam_nbest": 13}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
INVALID = 1
f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch


def test_symbols_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    src = open(HEADER).read()
    assert "#define TFASR_ABI_VERSION 44" in src
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name


def _rnnt_ws(B, T, U, J, V, W):
    n = ctypes.c_size_t(0)
    assert _lib.load().tfasr_rnnt_beam_workspace_size(B, T, U, J, V, W, ctypes.byref(n)) == 0
    return n.value


def test_transducer_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    B, C, Tcap, E, U, J, V, W = 2, 4, 20, 8, 16, 16, 5, 4
    need = _rnnt_ws(B, Tcap, U, J, V, W)

    def reset(B_=B, Tcap_=Tcap, W_=W, blank=0, ws=f, wsb=need):
        return lib.tfasr_rnnt_beam_reset(None, B_, Tcap_, U, J, V, W_, blank, ws, wsb, None)

    for kw in (dict(B_=0), dict(Tcap_=0), dict(W_=0), dict(W_=65), dict(blank=-1), dict(blank=V), dict(ws=None), dict(wsb=need - 1)):
        assert reset(**kw) == INVALID, kw

    def adv(emb=f, lng=f, lnb=f, packed=None, encj=f, nv=f, B_=B, C_=C, Tcap_=Tcap, E_=E, U_=U, W_=W, blank=0, after=C, ws=f, wsb=need):
        return lib.tfasr_rnnt_beam_advance(emb, f, f, f, lng, lnb, f, f, f, f, packed, encj, nv, B_, C_, Tcap_, E_, U_, J, V, W_, blank, 1e-3,
                                           after, ws, wsb, None)

    for kw in (dict(emb=None), dict(encj=None), dict(nv=None), dict(ws=None), dict(lng=None), dict(B_=0), dict(C_=0), dict(C_=Tcap + 1),
               dict(Tcap_=0), dict(E_=0), dict(W_=0), dict(W_=65), dict(blank=-1), dict(blank=V), dict(after=Tcap + 1), dict(after=-1),
               dict(packed=f, U_=24), dict(wsb=need - 1)):
        assert adv(**kw) == INVALID, kw

    def commit(com=f, toks=f, n=f, B_=B, W_=W, width=8, blank=0, ws=f, wsb=need):
        return lib.tfasr_rnnt_beam_commit(None, com, toks, n, B_, Tcap, U, J, V, W_, width, blank, ws, wsb, None)

    for kw in (dict(com=None), dict(toks=None), dict(n=None), dict(B_=0), dict(W_=65), dict(width=0), dict(blank=V), dict(ws=None),
               dict(wsb=need - 1)):
        assert commit(**kw) == INVALID, kw

    def nbest(NP=2, width=8, toks=f, nh=f, ws=f, wsb=need, W_=W, blank=0):
        return lib.tfasr_rnnt_beam_nbest_states(B, Tcap, U, J, V, W_, NP, blank, width, toks, f, f, f, nh, f, ws, wsb, None)

    for kw in (dict(NP=0), dict(NP=W + 1), dict(width=0), dict(width=Tcap + 1), dict(toks=None), dict(nh=None), dict(ws=None),
               dict(wsb=need - 1), dict(W_=0), dict(blank=V)):
        assert nbest(**kw) == INVALID, kw


def test_ctc_entries_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    B, C, Tcap, V, W = 3, 4, 19, 6, 8
    n = ctypes.c_size_t(0)
    assert lib.tfasr_ctc_beam_stream_workspace_size(B, C, Tcap, V, W, ctypes.byref(n)) == 0 and n.value > 0
    need = n.value
    for args in ((0, C, Tcap, V, W), (B, 0, Tcap, V, W), (B, Tcap + 1, Tcap, V, W), (B, C, 0, V, W), (B, C, Tcap, 1, W), (B, C, Tcap, V, 0),
                 (B, C, Tcap, V, 65)):
        assert lib.tfasr_ctc_beam_stream_workspace_size(*args, ctypes.byref(n)) == INVALID, args
    assert lib.tfasr_ctc_beam_stream_workspace_size(B, C, Tcap, V, W, None) == INVALID
    m = ctypes.c_size_t(0)
    assert lib.tfasr_ctc_beam_stream_workspace_size(B, C, 2 * Tcap, V, W, ctypes.byref(m)) == 0 and m.value > need  # the trie grows with Tcap

    def reset(B_=B, W_=W, ws=f, wsb=need):
        return lib.tfasr_ctc_beam_reset(None, B_, C, Tcap, V, W_, ws, wsb, None)

    for kw in (dict(B_=0), dict(W_=0), dict(W_=65), dict(ws=None), dict(wsb=need - 1)):
        assert reset(**kw) == INVALID, kw

    def adv(lg=f, nv=f, B_=B, Cn=C, W_=W, blank=V - 1, dtype=0, after=C, ws=f, wsb=need):
        return lib.tfasr_ctc_beam_advance(lg, nv, B_, C, Cn, Tcap, V, W_, blank, dtype, after, ws, wsb, None)

    for kw in (dict(lg=None), dict(nv=None), dict(B_=0), dict(Cn=0), dict(Cn=C + 1), dict(W_=0), dict(W_=65), dict(blank=-1), dict(blank=V),
               dict(dtype=2), dict(after=Tcap + 1), dict(after=-1), dict(ws=None), dict(wsb=need - 1)):
        assert adv(**kw) == INVALID, kw

    def commit(com=f, toks=f, n_=f, width=8, W_=W, ws=f, wsb=need):
        return lib.tfasr_ctc_beam_commit(None, com, toks, n_, B, C, Tcap, V, W_, width, ws, wsb, None)

    for kw in (dict(com=None), dict(toks=None), dict(n_=None), dict(width=0), dict(W_=65), dict(ws=None), dict(wsb=need - 1)):
        assert commit(**kw) == INVALID, kw

    def nbest(NP=2, width=8, toks=f, ws=f, wsb=need):
        return lib.tfasr_ctc_beam_nbest(B, C, Tcap, V, W, NP, width, toks, f, f, ws, wsb, None)

    for kw in (dict(NP=0), dict(NP=W + 1), dict(width=0), dict(width=Tcap + 1), dict(toks=None), dict(ws=None), dict(wsb=need - 1)):
        assert nbest(**kw) == INVALID, kw


def test_python_stream_classes_check_their_arguments_without_a_device():
    z = torch.zeros
    weights = [z(5, 8), z(8, 64), z(16, 64), z(64), None, None, z(16, 16), z(16), z(16, 5), z(5)]
    for kw in (dict(beam_width=0), dict(beam_width=65), dict(blank=5), dict(blank=-1)):
        with pytest.raises(ValueError):
            K.RnntBeamStream(weights, 2, 20, **dict(dict(beam_width=4, blank=0), **kw))
    with pytest.raises(ValueError):
        K.RnntBeamStream(weights, 2, 0, 4)
    for kw in (dict(beam_width=0), dict(beam_width=65), dict(blank_index=6), dict(C=0), dict(C=20)):
        a = dict(dict(B=2, C=4, Tcap=19, V=6, beam_width=4, blank_index=None, device="cpu"), **kw)
        with pytest.raises(ValueError):
            K.CtcBeamStream(**a)
    for cls in (K.RnntBeamStream, K.CtcBeamStream):
        for name in ("reset", "advance", "commit", "nbest"):
            assert callable(getattr(cls, name)), (cls, name)


def test_session_surface_and_argument_validation():
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC

    assert streaming.StreamOutput._fields == ("tokens", "tokens_length", "frames")
    for cls in (ConformerTransducer, ConformerCTC):
        params = list(inspect.signature(cls.stream).parameters)
        assert params == ["self", "batch_size", "precision", "max_tokens_per_frame", "beam_width", "max_frames"], params
        sig = inspect.signature(cls.stream)
        assert sig.parameters["beam_width"].default == 0 and sig.parameters["max_frames"].default == 3000
    assert callable(streaming.StreamingRecognizer.hypotheses)
    assert streaming.check_stream_args() == (1, 3, 0, 3000)
    assert streaming.check_stream_args(4, 1, 64, 1) == (4, 1, 64, 1)
    with pytest.raises(ValueError, match="beam_width"):
        streaming.check_stream_args(beam_width=65)
    with pytest.raises(ValueError, match="beam_width"):
        streaming.check_stream_args(beam_width=-1)
    with pytest.raises(ValueError, match="max_frames"):
        streaming.check_stream_args(max_frames=0)
    with pytest.raises(ValueError, match="batch_size"):
        streaming.check_stream_args(batch_size=0)
    doc = streaming.StreamingRecognizer.__doc__
    assert "max_tokens_per_frame=1" in doc and "max_frames" in doc and "bytes" in doc
