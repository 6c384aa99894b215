"""tfasr_edit_distance (scoring, ABI 44 additions): the symbols, the workspace query and the argument checks answer without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import metrics

NEW = {"tfasr_edit_distance_workspace_size": 4, "tfasr_edit_distance": 12}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
MAX_LEN = 4096  # TFASR_EDIT_MAX_LEN


def _ws(*dims):
    n = ctypes.c_size_t(0)
    st = _lib.load().tfasr_edit_distance_workspace_size(*dims, ctypes.byref(n))
    return st, n.value


def test_symbols_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    src = open(HEADER).read()
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert f"#define TFASR_EDIT_MAX_LEN {MAX_LEN}" in src and metrics.EDIT_MAX_LEN == MAX_LEN


@pytest.mark.parametrize("dims", [(0, 4, 4), (-1, 4, 4), (2, -1, 4), (2, 4, -1)])
def test_workspace_query_rejects_bad_shapes(dims):
    assert _ws(*dims)[0] == 1


def test_workspace_query_rejects_a_null_out_pointer_and_accepts_empty_widths():
    assert _lib.load().tfasr_edit_distance_workspace_size(2, 4, 4, None) == 1
    for dims in ((1, 0, 0), (3, 0, 7), (3, 7, 0), (1000, 40, 40)):
        st, n = _ws(*dims)
        assert st == 0 and n > 0, dims
    assert K.edit_distance_workspace_size(32, 200, 200) == _ws(32, 200, 200)[1]


def test_widths_beyond_the_kernels_are_unsupported_by_both_functions():
    assert _ws(1, MAX_LEN, MAX_LEN)[0] == 0
    assert _ws(1, MAX_LEN + 1, 8)[0] == _lib.STATUS_UNSUPPORTED and _ws(1, 8, MAX_LEN + 1)[0] == _lib.STATUS_UNSUPPORTED
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)  # never dereferenced
    big = 1 << 20
    assert lib.tfasr_edit_distance(f, f, f, f, 1, MAX_LEN + 1, 8, -1, f, f, big, None) == _lib.STATUS_UNSUPPORTED
    assert lib.tfasr_edit_distance(f, f, f, f, 1, 8, MAX_LEN + 1, -1, f, f, big, None) == _lib.STATUS_UNSUPPORTED
    with pytest.raises(_lib.TfasrUnsupported):
        K.edit_distance_workspace_size(1, MAX_LEN + 1, 8)


def test_invalid_arguments_are_rejected_without_touching_the_gpu():
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch
    P, N, M = 3, 9, 7
    _, need = _ws(P, N, M)

    def call(hyp=f, hl=f, ref=f, rl=f, P_=P, N_=N, M_=M, skip=-1, out=f, ws=f, wsb=need):
        return lib.tfasr_edit_distance(hyp, hl, ref, rl, P_, N_, M_, skip, out, ws, wsb, None)

    for kw in (dict(hyp=None), dict(ref=None), dict(out=None), dict(ws=None), dict(P_=0), dict(P_=-2), dict(N_=-1), dict(M_=-1),
               dict(wsb=need - 1), dict(wsb=0), dict(hyp=None, hl=None), dict(ref=None, rl=None)):
        assert call(**kw) == 1, kw


def test_python_wrappers_refuse_cpu_tensors():
    i32 = torch.int32
    with pytest.raises(_lib.TfasrError):
        K.edit_distance(torch.zeros(2, 3, dtype=i32), torch.zeros(2, 3, dtype=i32))
    with pytest.raises(_lib.TfasrError):
        K.edit_distance(torch.zeros(2, 3, dtype=i32), torch.zeros(2, 3, dtype=i32), torch.ones(2, dtype=i32), torch.ones(2, dtype=i32), skip_id=0)
    # the metrics front end is where CPU data belongs: it goes to the host routine
    out = metrics.edit_distance(torch.tensor([[0, 1]], dtype=i32), torch.tensor([[1, 0]], dtype=i32), torch.tensor([2]), torch.tensor([2]))
    assert [int(c[0]) for c in out] == [2, 1, 0, 1, 1]
    out = metrics.edit_distance(np.array([[0, 1]]), np.array([[1, 0]]), [2], [2])
    assert [int(c[0]) for c in out] == [2, 1, 0, 1, 1]


def test_metrics_and_model_surface():
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.contextnet import ContextNetTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC

    assert metrics.EditCounts._fields == ("distance", "hits", "substitutions", "deletions", "insertions")
    for name in ("edit_distance", "edit_distance_host", "encode_pairs", "ErrorStats", "evaluate_hypotheses"):
        assert callable(getattr(metrics, name)), name
    import inspect

    for cls in (ConformerTransducer, ContextNetTransducer, ConformerCTC):
        assert callable(cls.evaluate)
        params = list(inspect.signature(cls.evaluate).parameters)
        assert params[:9] == ["self", "data", "output_file_path", "names", "beam_width", "top_paths", "device_search", "cer_unit", "device_metrics"]
