"""tfasr_ctc_greedy_decode_carry_detail (declared under ABI 44) and the detail sessions' surface: the symbol, the wrapper, the host-side
argument checks and the session arguments answer without a GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tensorflowasr_amd import _lib, streaming
from tensorflowasr_amd import kernels as K

NAME = "tfasr_ctc_greedy_decode_carry_detail"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
INVALID = 1
f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch
POINTERS = ("logits", "logit_len", "final", "state_i", "state_f", "tokens", "tokens_len", "starts", "ends", "tok_logp", "tok_entropy")


def test_symbol_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    src = open(HEADER).read()
    assert "#define TFASR_ABI_VERSION 44" in src
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == len(POINTERS) + 6  # + B, C, V, blank, dtype, stream
    assert callable(K.ctc_greedy_decode_carry_detail) and callable(K.CtcDetailState.reset)
    assert len(_lib.SIGNATURES["tfasr_ctc_greedy_decode_carry"][1]) == 12  # the plain carried decoder keeps its signature


def _call(B=2, C=16, V=29, blank=0, dtype=0, **ptr):
    args = [ptr.get(name, f) for name in POINTERS]
    return _lib.load().tfasr_ctc_greedy_decode_carry_detail(*args, B, C, V, blank, dtype, None)


def test_bad_arguments_are_refused_on_the_host():
    for name in POINTERS:
        assert _call(**{name: None}) == INVALID, name
    for kw in (dict(B=0), dict(B=-1), dict(C=0), dict(C=-4), dict(V=1), dict(V=0), dict(blank=-1), dict(blank=29), dict(blank=2, V=2), dict(dtype=2),
               dict(dtype=-1)):
        assert _call(**kw) == INVALID, kw


def test_wrapper_refuses_cpu_tensors_and_a_state_of_another_size():
    i = torch.zeros(2, dtype=torch.int32)
    st = K.CtcDetailState(2, "cpu")
    assert st.ints.tolist() == [[-1, 0, 0, 0]] * 2 and st.floats.tolist() == [[0.0] * 3] * 2
    st.ints[:] = 7
    st.floats[:] = 1.5
    st.reset([1])
    assert st.ints.tolist() == [[7] * 4, [-1, 0, 0, 0]] and st.floats.tolist() == [[1.5] * 3, [0.0] * 3]
    assert st.seen.tolist() == [7, 0] and st.open.tolist() == [True, False] and st.score.tolist() == [1.5, 0.0]
    with pytest.raises(_lib.TfasrError, match="device"):
        K.ctc_greedy_decode_carry_detail(torch.zeros(2, 5, 7), i, st)
    with pytest.raises(ValueError, match="state of 3 streams"):
        K.ctc_greedy_decode_carry_detail(torch.zeros(2, 5, 7), i, K.CtcDetailState(3, "cpu"))
    with pytest.raises(ValueError, match="logit_len"):
        K.ctc_greedy_decode_carry_detail(torch.zeros(2, 5, 7), i.long(), st)
    with pytest.raises(ValueError, match="final"):
        K.ctc_greedy_decode_carry_detail(torch.zeros(2, 5, 7), i, st, final=torch.zeros(3, dtype=torch.int32))


def test_stream_outputs_keep_their_fields():
    assert streaming.StreamOutput._fields == ("tokens", "tokens_length", "frames")
    assert streaming.StreamDetailOutput._fields[:3] == streaming.StreamOutput._fields
    assert streaming.StreamDetailOutput._fields[3:] == ("token_frames", "token_ends", "log_probs", "entropies")


def test_every_streamable_class_opens_detail_sessions_and_stream_keeps_its_signature():
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.contextnet import ContextNetTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC
    from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC
    from tensorflowasr_amd.jasper import JasperCTC
    from tensorflowasr_amd.rnnt import RnnTransducer
    from tensorflowasr_amd.transformer import TransformerCTC, TransformerTransducer

    for cls in (ConformerTransducer, ConformerCTC, TransformerCTC, TransformerTransducer, JasperCTC, DeepSpeech2CTC, RnnTransducer):
        assert cls.stream_detailed is ConformerTransducer.stream_detailed, cls  # one door, the arguments of the class's own stream()
        assert "detail" not in inspect.signature(cls.stream).parameters, cls
    with pytest.raises(NotImplementedError, match="ContextNet cannot stream"):
        ContextNetTransducer.stream_detailed(object.__new__(ContextNetTransducer), 2)
    p = list(inspect.signature(streaming.StreamingRecognizer.__init__).parameters.values())[-1]
    assert p.name == "detail" and p.default is False
    assert callable(streaming.StreamingRecognizer.detailed)


class _Fresh:  # what detailed() reads of a session before it re-initialises its search state
    def __init__(self, beam_width, total=(0, 0), chunks_run=0):
        self.beam_width, self.total, self.chunks_run, self.B, self.detail = beam_width, list(total), chunks_run, len(total), False

    _check_detail = streaming.StreamingRecognizer._check_detail


def test_detail_with_a_beam_is_refused_with_the_reason():
    with pytest.raises(ValueError, match="beam sessions keep their outputs"):
        streaming.StreamingRecognizer(None, 1, beam_width=1, detail=True)
    with pytest.raises(ValueError, match="beam sessions keep their outputs"):
        streaming.StreamingRecognizer.detailed(_Fresh(beam_width=4))
    for late in (_Fresh(0, total=(0, 160)), _Fresh(0, chunks_run=1)):
        with pytest.raises(RuntimeError, match="before the first accept"):
            streaming.StreamingRecognizer.detailed(late)
