"""tfasr_rnnt_beam_* (device transducer beam search, ABI 44 additions): the symbols, the workspace query and the argument checks
answer without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

NEW = {"tfasr_rnnt_beam_workspace_size": 7, "tfasr_rnnt_beam_search": 35, "tfasr_rnnt_beam_begin": 11, "tfasr_rnnt_beam_select": 13,
       "tfasr_rnnt_beam_nbest": 14}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")


def _ws(B, T, U, J, V, W):
    n = ctypes.c_size_t(0)
    st = _lib.load().tfasr_rnnt_beam_workspace_size(B, T, U, J, V, W, ctypes.byref(n))
    return st, n.value


def test_symbols_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    src = open(HEADER).read()
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name


def test_workspace_size_grows_with_every_dimension():
    base_args = (4, 50, 24, 40, 29, 4)
    st, base = _ws(*base_args)
    assert st == 0 and base > 0
    for i, bigger in ((0, 8), (1, 100), (2, 48), (4, 1000), (5, 16)):  # B, T, U, V, W
        args = list(base_args)
        args[i] = bigger
        st, n = _ws(*args)
        assert st == 0 and n > base, args
    st, n = _ws(32, 250, 640, 640, 1000, 10)  # the bench shape
    assert st == 0 and n < 256 << 20


@pytest.mark.parametrize("args", [(0, 10, 8, 8, 5, 2), (2, 0, 8, 8, 5, 2), (2, 10, 0, 8, 5, 2), (2, 10, 8, 0, 5, 2), (2, 10, 8, 8, 1, 2),
                                  (2, 10, 8, 8, 5, 0), (2, 10, 8, 8, 5, 65)])
def test_workspace_size_rejects_bad_shapes(args):
    assert _ws(*args)[0] != 0
    assert _lib.load().tfasr_rnnt_beam_workspace_size(2, 10, 8, 8, 5, 2, None) != 0


def test_invalid_search_arguments_return_nonzero_without_touching_the_gpu():
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch
    B, T, E, U, J, V = 2, 10, 8, 16, 16, 5
    _, need = _ws(B, T, U, J, V, 4)

    def call(W=4, NP=2, blank=0, V_=V, E_=E, U_=U, lng=f, lnb=f, ih=f, ic=f, packed=None, enc=f, nfr=f, toks=f, ws=f, wsb=need, nh=f):
        return lib.tfasr_rnnt_beam_search(f, f, f, f, lng, lnb, f, f, f, f, packed, enc, nfr, f, ih, ic, B, T, E_, U_, J, V_, W, NP, blank,
                                          1e-3, toks, f, f, f, nh, f, ws, wsb, None)

    assert call(enc=None) != 0 and call(nfr=None) != 0 and call(toks=None) != 0 and call(ws=None) != 0 and call(nh=None) != 0
    assert call(lng=None) != 0 and call(ih=None) != 0  # LayerNorm gamma / beta and h / c come in pairs
    assert call(W=0) != 0 and call(W=65) != 0
    assert call(NP=0) != 0 and call(NP=5) != 0
    assert call(blank=-1) != 0 and call(blank=V) != 0
    assert call(V_=1, blank=0) != 0
    assert call(E_=0) != 0 and call(U_=0) != 0
    assert call(packed=f, U_=24) != 0  # decode_pack makes no G for U % 16 != 0
    assert call(wsb=need - 1) != 0


def test_invalid_seam_arguments_return_nonzero_without_touching_the_gpu():
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)
    B, T, V, W = 2, 10, 5, 4
    _, need = _ws(B, T, 1, 1, V, W)
    assert lib.tfasr_rnnt_beam_begin(None, B, T, 1, 1, V, W, V, f, need, None) != 0
    assert lib.tfasr_rnnt_beam_begin(None, B, T, 1, 1, V, 65, 0, f, need, None) != 0
    assert lib.tfasr_rnnt_beam_begin(None, B, T, 1, 1, V, W, 0, None, need, None) != 0
    assert lib.tfasr_rnnt_beam_begin(None, B, T, 1, 1, V, W, 0, f, need - 1, None) != 0
    sel = lambda lg=f, nf=f, t=0, blank=0, ws=f, wsb=need: lib.tfasr_rnnt_beam_select(lg, nf, t, B, T, 1, 1, V, W, blank, ws, wsb, None)
    assert sel(lg=None) != 0 and sel(nf=None) != 0 and sel(ws=None) != 0
    assert sel(t=-1) != 0 and sel(t=T) != 0 and sel(blank=V) != 0 and sel(wsb=need - 1) != 0
    nb = lambda NP=2, toks=f, ws=f: lib.tfasr_rnnt_beam_nbest(B, T, 1, 1, V, W, NP, 0, toks, f, f, ws, need, None)
    assert nb(NP=0) != 0 and nb(NP=W + 1) != 0 and nb(toks=None) != 0 and nb(ws=None) != 0


def _weights(V=5, E=8, U=16, J=16):
    z = torch.zeros
    return [z(V, E), z(E, 4 * U), z(U, 4 * U), z(4 * U), None, None, z(U, J), z(J), z(J, V), z(V)]


@pytest.mark.parametrize("kw", [dict(beam_width=0), dict(beam_width=65), dict(beam_width=4, top_paths=5), dict(top_paths=0),
                                dict(blank=-1), dict(blank=5)])
def test_python_wrappers_raise_value_error(kw):
    kw = dict(dict(beam_width=4, top_paths=1, blank=0), **kw)
    with pytest.raises(ValueError):
        K.rnnt_beam_search(*_weights(), torch.zeros(2, 10, 16), torch.tensor([10, 3], dtype=torch.int32), **kw)
    if "top_paths" not in kw or kw["top_paths"] == 1:
        with pytest.raises(ValueError):
            K.rnnt_beam_begin(2, 10, 5, kw["beam_width"], kw["blank"], device="cpu")


def test_ctc_model_has_no_transducer_beam_search():
    from tensorflowasr_amd.ctc_model import ConformerCTC

    with pytest.raises(NotImplementedError):
        ConformerCTC.recognize_beam_encoded(object.__new__(ConformerCTC), None, None, 4, 1)
