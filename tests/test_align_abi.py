"""tfasr_rnnt_align* / tfasr_ctc_align (forced alignment, ABI 44 additions): the symbols, the workspace queries and the argument
checks answer without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

NEW = {"tfasr_rnnt_align_workspace_size": 5, "tfasr_ctc_align_workspace_size": 5, "tfasr_rnnt_align_lattice": 15, "tfasr_rnnt_align": 18,
       "tfasr_rnnt_align_stats": 19, "tfasr_ctc_align": 18}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
MAX_U1, CTC_MAX_U = 1024, 511  # TFASR_ALIGN_MAX_U1, TFASR_ALIGN_CTC_MAX_U


def _ws(fn, *dims):
    n = ctypes.c_size_t(0)
    st = getattr(_lib.load(), fn)(*dims, ctypes.byref(n))
    return st, n.value


def test_symbols_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    src = open(HEADER).read()
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert f"#define TFASR_ALIGN_MAX_U1 {MAX_U1}" in src and f"#define TFASR_ALIGN_CTC_MAX_U {CTC_MAX_U}" in src


@pytest.mark.parametrize("fn", ["tfasr_rnnt_align_workspace_size", "tfasr_ctc_align_workspace_size"])
def test_workspace_size_grows_with_every_dimension(fn):
    """B, T and the label width each enlarge the workspace; the vocabulary is no dimension of it (one bit, or two, per lattice node
    and three floats per node for the log-probabilities), so V must not shrink it."""
    base_args = (4, 50, 24, 29)
    st, base = _ws(fn, *base_args)
    assert st == 0 and base > 0
    for i, bigger in ((0, 8), (1, 100), (2, 48)):
        args = list(base_args)
        args[i] = bigger
        st, n = _ws(fn, *args)
        assert st == 0 and n > base, args
    st, n = _ws(fn, 4, 50, 24, 1000)
    assert st == 0 and n >= base


def test_workspace_stays_small_at_the_bench_shapes():
    for T, U1 in ((250, 65), (743, 200)):
        st, n = _ws("tfasr_rnnt_align_workspace_size", 32, T, U1, 1000)
        assert st == 0 and 0 < n < 256 << 20, (T, U1, n)
        st, n = _ws("tfasr_ctc_align_workspace_size", 32, T, U1 - 1, 1000)
        assert st == 0 and 0 < n < 256 << 20, (T, U1, n)
    assert K.rnnt_align_workspace_size(32, 250, 65, 1000) == _ws("tfasr_rnnt_align_workspace_size", 32, 250, 65, 1000)[1]
    assert K.ctc_align_workspace_size(32, 250, 64, 1000) == _ws("tfasr_ctc_align_workspace_size", 32, 250, 64, 1000)[1]


@pytest.mark.parametrize("args", [(0, 10, 8, 5), (2, 0, 8, 5), (2, 10, 0, 5), (2, 10, 8, 0), (-1, 10, 8, 5)])
def test_rnnt_workspace_size_rejects_bad_shapes(args):
    assert _ws("tfasr_rnnt_align_workspace_size", *args)[0] == 1
    assert _lib.load().tfasr_rnnt_align_workspace_size(2, 10, 8, 5, None) == 1


@pytest.mark.parametrize("args", [(0, 10, 8, 5), (2, 0, 8, 5), (2, 10, -1, 5), (2, 10, 8, 0)])
def test_ctc_workspace_size_rejects_bad_shapes(args):
    assert _ws("tfasr_ctc_align_workspace_size", *args)[0] == 1
    assert _lib.load().tfasr_ctc_align_workspace_size(2, 10, 8, 5, None) == 1


def test_widths_beyond_the_kernels_are_unsupported():
    assert _ws("tfasr_rnnt_align_workspace_size", 1, 4, MAX_U1, 5)[0] == 0
    assert _ws("tfasr_rnnt_align_workspace_size", 1, 4, MAX_U1 + 1, 5)[0] == _lib.STATUS_UNSUPPORTED
    assert _ws("tfasr_ctc_align_workspace_size", 1, 4, CTC_MAX_U, 5)[0] == 0
    assert _ws("tfasr_ctc_align_workspace_size", 1, 4, CTC_MAX_U + 1, 5)[0] == _lib.STATUS_UNSUPPORTED
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)
    big = 1 << 30
    assert lib.tfasr_rnnt_align_lattice(f, f, f, f, None, 0, 1, 4, MAX_U1 + 1, f, f, f, f, big, None) == _lib.STATUS_UNSUPPORTED
    assert lib.tfasr_rnnt_align(f, f, f, f, None, 0, 1, 4, MAX_U1 + 1, 5, 0, 0, f, f, f, f, big, None) == _lib.STATUS_UNSUPPORTED
    assert lib.tfasr_rnnt_align_stats(f, 2, f, f, f, f, None, 0, 1, 4, MAX_U1 + 1, 5, 0, f, f, f, f, big, None) == _lib.STATUS_UNSUPPORTED
    assert lib.tfasr_ctc_align(f, f, f, f, 1, 4, CTC_MAX_U + 1, 5, 0, 0, 0, f, f, f, f, f, big, None) == _lib.STATUS_UNSUPPORTED


def test_invalid_transducer_arguments_are_rejected_without_touching_the_gpu():
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch
    B, T, U1, V = 2, 10, 5, 7
    _, need = _ws("tfasr_rnnt_align_workspace_size", B, T, U1, V)

    def lattice(bl=f, tr=f, ul=f, tl=f, off=None, total=0, B_=B, T_=T, U1_=U1, fr=f, lp=f, sc=f, ws=f, wsb=need):
        return lib.tfasr_rnnt_align_lattice(bl, tr, ul, tl, off, total, B_, T_, U1_, fr, lp, sc, ws, wsb, None)

    for kw in (dict(bl=None), dict(tr=None), dict(ul=None), dict(tl=None), dict(fr=None), dict(lp=None), dict(sc=None), dict(ws=None),
               dict(B_=0), dict(T_=0), dict(U1_=0), dict(wsb=64), dict(off=f, total=0), dict(off=f, total=B * T * U1 + 1)):
        assert lattice(**kw) == 1, kw

    def full(lg=f, lab=f, ul=f, tl=f, off=None, total=0, B_=B, T_=T, U1_=U1, V_=V, blank=0, dtype=0, fr=f, lp=f, sc=f, ws=f, wsb=need):
        return lib.tfasr_rnnt_align(lg, lab, ul, tl, off, total, B_, T_, U1_, V_, blank, dtype, fr, lp, sc, ws, wsb, None)

    for kw in (dict(lg=None), dict(lab=None), dict(ul=None), dict(tl=None), dict(fr=None), dict(lp=None), dict(sc=None), dict(ws=None),
               dict(B_=0), dict(T_=0), dict(U1_=0), dict(V_=1), dict(V_=0), dict(blank=-1), dict(blank=V), dict(dtype=2), dict(wsb=need - 1),
               dict(off=f, total=0), dict(off=f, total=B * T * U1 + 1)):
        assert full(**kw) == 1, kw
    assert full(blank=1) == _lib.STATUS_UNSUPPORTED  # the lattice log-probabilities take the blank from column 0, as the loss

    def stats(part=f, nparts=2, pick=f, lab=f, ul=f, tl=f, off=None, total=0, V_=V, blank=0, fr=f, sc=f, ws=f, wsb=need):
        return lib.tfasr_rnnt_align_stats(part, nparts, pick, lab, ul, tl, off, total, B, T, U1, V_, blank, fr, f, sc, ws, wsb, None)

    for kw in (dict(part=None), dict(nparts=0), dict(pick=None), dict(lab=None), dict(ul=None), dict(tl=None), dict(fr=None), dict(sc=None),
               dict(ws=None), dict(V_=1), dict(blank=-1), dict(blank=V), dict(wsb=need - 1), dict(off=f, total=-3)):
        assert stats(**kw) == 1, kw


def test_invalid_ctc_arguments_are_rejected_without_touching_the_gpu():
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)
    B, T, U, V = 2, 10, 4, 7
    _, need = _ws("tfasr_ctc_align_workspace_size", B, T, U, V)

    def call(lg=f, lab=f, ul=f, tl=f, B_=B, T_=T, U_=U, V_=V, blank=0, dtype=0, norm=0, st=f, en=f, lp=f, sc=f, ws=f, wsb=need):
        return lib.tfasr_ctc_align(lg, lab, ul, tl, B_, T_, U_, V_, blank, dtype, norm, st, en, lp, sc, ws, wsb, None)

    for kw in (dict(lg=None), dict(lab=None), dict(ul=None), dict(tl=None), dict(st=None), dict(en=None), dict(lp=None), dict(sc=None),
               dict(ws=None), dict(B_=0), dict(T_=0), dict(U_=-1), dict(V_=1), dict(blank=-1), dict(blank=V), dict(dtype=2), dict(wsb=need - 1)):
        assert call(**kw) == 1, kw


def test_python_wrappers_refuse_cpu_tensors_and_wide_labels():
    i32 = torch.int32
    with pytest.raises(Exception):
        K.rnnt_align_lattice(torch.zeros(1, 3, 2), torch.zeros(1, 3, 2), torch.ones(1, dtype=i32), torch.ones(1, dtype=i32))
    with pytest.raises(Exception):
        K.ctc_align(torch.zeros(1, 3, 4), torch.ones(1, 1, dtype=i32), torch.ones(1, dtype=i32), torch.ones(1, dtype=i32))
    with pytest.raises(_lib.TfasrError):  # the width is refused by the workspace query, before any device pointer is needed
        K.rnnt_align_lattice(torch.zeros(1, 2, MAX_U1 + 1), torch.zeros(1, 2, MAX_U1 + 1), torch.ones(1, dtype=i32), torch.ones(1, dtype=i32))


def test_schema_and_model_surface():
    from tensorflowasr_amd import schemas
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.contextnet import ContextNetTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC

    assert schemas.AlignOutput._fields == ("frames", "ends", "label_log_probs", "scores", "seconds_per_frame")
    for cls in (ConformerTransducer, ContextNetTransducer, ConformerCTC):
        assert callable(cls.align) and callable(cls.align_encoded)
    with pytest.raises(NotImplementedError):
        ConformerCTC.align_encoded(object.__new__(ConformerCTC), None, None, None, None, None)
    out = schemas.AlignOutput(torch.tensor([[0, 3, -1]], dtype=torch.int32), None, torch.zeros(1, 3), torch.zeros(1), 0.04)
    assert schemas.token_times(out).tolist() == [[0.0, pytest.approx(0.12), -1.0]]
