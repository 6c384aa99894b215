"""tfasr_row_lse_entropy / tfasr_ctc_nbest_align* (token times and confidences of n-best lists, ABI 44 additions): the symbols, the
workspace query and the argument checks answer without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

NEW = {"tfasr_row_lse_entropy": 7, "tfasr_ctc_nbest_align_workspace_size": 6, "tfasr_ctc_nbest_align": 20}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
CTC_MAX_U = 511  # TFASR_ALIGN_CTC_MAX_U


def _ws(*dims):
    n = ctypes.c_size_t(0)
    st = _lib.load().tfasr_ctc_nbest_align_workspace_size(*dims, ctypes.byref(n))
    return st, n.value


def test_symbols_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    src = open(HEADER).read()
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert K.ALIGN_CTC_MAX_U == CTC_MAX_U and f"#define TFASR_ALIGN_CTC_MAX_U {CTC_MAX_U}" in src


def test_workspace_size_depends_on_its_arguments_only():
    base_args = (4, 4, 50, 24, 29)
    st, base = _ws(*base_args)
    assert st == 0 and base > 0 and _ws(*base_args) == (0, base)
    for i, bigger in ((0, 8), (1, 8), (2, 100), (3, 48)):
        args = list(base_args)
        args[i] = bigger
        st, n = _ws(*args)
        assert st == 0 and n > base, args
    assert _ws(4, 4, 50, 24, 1000) == (0, base)  # the vocabulary is no dimension of it
    assert K.ctc_nbest_align_workspace_size(*base_args) == base
    # the frame statistics are held once per utterance: P paths cost less than P utterances
    assert _ws(4, 4, 50, 24, 29)[1] < _ws(16, 1, 50, 24, 29)[1]
    st, n = _ws(32, 4, 250, 250, 1000)
    assert st == 0 and 0 < n < 64 << 20


@pytest.mark.parametrize("args", [(0, 2, 10, 8, 5), (2, 0, 10, 8, 5), (2, 2, 0, 8, 5), (2, 2, 10, -1, 5), (2, 2, 10, 8, 0)])
def test_workspace_size_rejects_bad_shapes(args):
    assert _ws(*args)[0] == 1
    assert _lib.load().tfasr_ctc_nbest_align_workspace_size(2, 2, 10, 8, 5, None) == 1


def test_widths_beyond_the_kernel_are_unsupported():
    assert _ws(1, 2, 4, CTC_MAX_U, 5)[0] == 0
    assert _ws(1, 2, 4, CTC_MAX_U + 1, 5)[0] == _lib.STATUS_UNSUPPORTED
    f = ctypes.c_void_p(0x1000)
    assert _lib.load().tfasr_ctc_nbest_align(f, f, f, 600, f, 1, 2, 4, 512, 5, 0, 0, f, f, f, f, f, f, 1 << 30, None) == _lib.STATUS_UNSUPPORTED


def test_invalid_arguments_are_rejected_without_touching_the_gpu():
    lib = _lib.load()
    f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch
    B, P, T, U, V = 2, 3, 10, 4, 7
    _, need = _ws(B, P, T, U, V)

    def call(lg=f, tl=f, lab=f, ldl=T, ul=f, B_=B, P_=P, T_=T, U_=U, V_=V, blank=0, dtype=0, st=f, en=f, lp=f, ent=f, sc=f, ws=f, wsb=need):
        return lib.tfasr_ctc_nbest_align(lg, tl, lab, ldl, ul, B_, P_, T_, U_, V_, blank, dtype, st, en, lp, ent, sc, ws, wsb, None)

    for kw in (dict(lg=None), dict(tl=None), dict(lab=None), dict(ul=None), dict(st=None), dict(en=None), dict(lp=None), dict(ent=None),
               dict(sc=None), dict(ws=None), dict(ldl=U - 1), dict(B_=0), dict(P_=0), dict(T_=0), dict(U_=-1), dict(V_=1), dict(blank=-1),
               dict(blank=V), dict(dtype=2), dict(wsb=need - 1), dict(wsb=0)):
        assert call(**kw) == 1, kw
    assert call(U_=512, ldl=512, wsb=1 << 30) == _lib.STATUS_UNSUPPORTED

    def stats(x=f, rows=8, V_=V, dtype=0, lse=f, ent=f):
        return lib.tfasr_row_lse_entropy(x, rows, V_, dtype, lse, ent, None)

    for kw in (dict(x=None), dict(lse=None), dict(rows=0), dict(V_=0), dict(dtype=2), dict(dtype=-1)):
        assert stats(**kw) == 1, kw


def test_python_wrappers_refuse_cpu_tensors():
    i32 = torch.int32
    with pytest.raises(Exception):
        K.row_lse_entropy(torch.zeros(3, 4))
    with pytest.raises(Exception):
        K.ctc_nbest_align(torch.zeros(1, 3, 4), torch.ones(1, dtype=i32), torch.ones(1, 2, 3, dtype=i32), torch.ones(1, 2, dtype=i32))
    with pytest.raises(_lib.TfasrUnsupported):  # refused by the workspace query, before any device pointer is needed
        K.ctc_nbest_align(torch.zeros(1, 600, 4), torch.ones(1, dtype=i32), torch.ones(1, 2, 600, dtype=i32), torch.ones(1, 2, dtype=i32),
                          max_labels=CTC_MAX_U + 1)


def test_schema_and_model_surface():
    from tensorflowasr_amd import schemas
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.contextnet import ContextNetTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC, CtcModel
    from tensorflowasr_amd.transducer import TransducerModel

    assert schemas.NBestOutput._fields == ("search", "tokens", "lengths", "frames", "ends", "log_probs", "entropies", "path_scores",
                                           "seconds_per_frame", "vocab_size")
    for cls in (ConformerTransducer, ContextNetTransducer):
        assert cls.recognize_nbest_detailed is TransducerModel.recognize_nbest_detailed
    assert ConformerCTC.recognize_nbest_detailed is CtcModel.recognize_nbest_detailed
    tok = torch.tensor([[[3, 4, 0], [5, 0, 0]]], dtype=torch.int32)
    fr = torch.tensor([[[1, 4, -1], [2, -1, -1]]], dtype=torch.int32)
    lp = torch.tensor([[[-0.5, -1.0, 0.0], [-2.0, 0.0, 0.0]]])
    nb = schemas.NBestOutput((tok,), tok, torch.tensor([[2, 1]], dtype=torch.int32), fr, fr + 2, lp, torch.zeros(1, 2, 3),
                             torch.tensor([[-3.0, -4.0]]), 0.04, 29)
    p1 = nb.path(1)
    assert isinstance(p1, schemas.RecognizeOutput) and p1.predict.tokens.tolist() == [[5, 0, 0]] and p1.scores.tolist() == [-4.0]
    assert schemas.token_times(p1).tolist() == [[pytest.approx(0.08), -1.0, -1.0]]
    assert schemas.token_confidences(nb.path(0)).tolist() == [[pytest.approx(0.7788, abs=1e-4), pytest.approx(0.6065, abs=1e-4), 0.0]]
    tr = nb._replace(ends=None).path(0)
    assert tr.ends is None and schemas.token_confidences(tr)[0, 0].item() == pytest.approx(0.6065, abs=1e-4)
