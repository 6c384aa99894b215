"""tfasr_ctc_beam_search (device prefix beam search, ABI 44): the workspace query and the argument checks answer without a GPU."""
import ctypes

import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K


def _ws(B, T, V, W):
    n = ctypes.c_size_t(0)
    st = _lib.load().tfasr_ctc_beam_search_workspace_size(B, T, V, W, ctypes.byref(n))
    return st, n.value


def test_abi_version_and_symbols():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    assert "tfasr_ctc_beam_search" in _lib.SIGNATURES and "tfasr_ctc_beam_search_workspace_size" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["tfasr_ctc_beam_search"][1]) == 15


def test_workspace_size_grows_with_batch_frames_and_beam():
    st, base = _ws(4, 50, 29, 4)
    assert st == 0 and base > 0
    for args in ((8, 50, 29, 4), (4, 100, 29, 4), (4, 50, 29, 16)):
        st, n = _ws(*args)
        assert st == 0 and n > base, args
    st, n = _ws(32, 250, 1000, 10)  # the bench shape: a few MB
    assert st == 0 and n < 64 << 20


@pytest.mark.parametrize("args", [(0, 10, 5, 2), (2, 0, 5, 2), (2, 10, 1, 2), (2, 10, 5, 0), (2, 10, 5, 65)])
def test_workspace_size_rejects_bad_shapes(args):
    assert _ws(*args)[0] != 0
    assert _lib.load().tfasr_ctc_beam_search_workspace_size(2, 10, 5, 2, None) != 0


def test_invalid_arguments_return_nonzero_without_touching_the_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch
    B, T, V = 2, 10, 5
    _, need = _ws(B, T, V, 4)

    def call(logits=fake, llen=fake, W=4, P=1, blank=0, dtype=0, toks=fake, tlen=fake, lp=fake, ws=fake, wsb=need, V_=V):
        return lib.tfasr_ctc_beam_search(logits, llen, B, T, V_, W, P, blank, dtype, toks, tlen, lp, ws, wsb, None)

    assert call(logits=None) != 0
    assert call(llen=None) != 0
    assert call(toks=None) != 0 and call(tlen=None) != 0 and call(lp=None) != 0 and call(ws=None) != 0
    assert call(W=0) != 0 and call(W=65) != 0
    assert call(P=0) != 0 and call(P=5) != 0
    assert call(blank=-1) != 0 and call(blank=V) != 0
    assert call(V_=1, blank=0) != 0
    assert call(dtype=7) != 0
    assert call(wsb=need - 1) != 0


@pytest.mark.parametrize("kw", [dict(beam_width=0), dict(beam_width=65), dict(beam_width=4, top_paths=5), dict(top_paths=0),
                                dict(blank_index=-1), dict(blank_index=5)])
def test_python_entry_raises_value_error(kw):
    logits = torch.zeros(2, 10, 5)
    with pytest.raises(ValueError):
        K.ctc_beam_search_device(logits, torch.tensor([10, 3], dtype=torch.int32), **kw)
    with pytest.raises(ValueError):
        K.ctc_beam_search_device(torch.zeros(2, 10, 1), torch.tensor([10, 3], dtype=torch.int32), blank_index=0)
