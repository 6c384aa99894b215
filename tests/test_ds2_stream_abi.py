"""The DeepSpeech2 session's entry points (tfasr_lstm_infer_fwd_state, tfasr_stream_rowconv_fwd; declarations added under ABI 44, nothing
existing changes): the symbols, the answers the library gives on the host before any launch, conv2d_fwd's `lead` rule, the model surface
and check_streamable's DeepSpeech2 branch.  Nothing here needs a GPU."""
import ctypes
import inspect
import os
import re

import pytest

from tensorflowasr_amd import _lib, configs, streaming
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC
from tensorflowasr_amd.jasper import JasperCTC

NEW = {"tfasr_lstm_infer_fwd_state": 18, "tfasr_stream_rowconv_fwd": 13}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
INVALID, UNSUPPORTED = 1, _lib.STATUS_UNSUPPORTED
f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch


def _at(addr):
    return ctypes.c_void_p(addr)


def test_symbols_declared_and_exported():
    lib = _lib.load()
    src = open(HEADER).read()
    assert lib.tfasr_abi_version() == _lib.ABI_VERSION
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert callable(K.stream_rowconv_fwd)
    assert {"state", "state_out"} <= set(inspect.signature(K.lstm_infer_fwd).parameters)
    assert inspect.signature(K.conv2d_fwd).parameters["lead"].default == 0


# Every call below has a shape that is too large for the entry (B * T * 4P past 2^39 elements: UNSUPPORTED, answered on the host), and
# is otherwise legal.  The state's rules are judged first - an argument that is wrong wins over a size that is merely too large - so a
# call whose state passes answers UNSUPPORTED and one whose state is refused answers INVALID: each assertion depends on the one rule it
# names, and no call can end in a launch.
BIG = dict(B=65536, T=100000, P=32)
N = BIG["B"] * BIG["P"] * 4  # bytes of one [B, P] f32 state
H0, C0, HL, CL = 0x10000000, 0x20000000, 0x30000000, 0x40000000


def _lstm(xg=f, rk=f, lengths=f, y=f, h0=_at(H0), c0=_at(C0), h_last=_at(HL), c_last=_at(CL), B=BIG["B"], T=BIG["T"], P=BIG["P"], ndir=1,
          dtype=1, ws=f, ws_bytes=1 << 40, entry="tfasr_lstm_infer_fwd_state"):
    lib = _lib.load()
    if entry == "tfasr_lstm_infer_fwd":
        return lib.tfasr_lstm_infer_fwd(xg, ndir * 4 * P, rk, lengths, y, ndir * P, h_last, c_last, B, T, P, ndir, dtype, ws, ws_bytes, None)
    return lib.tfasr_lstm_infer_fwd_state(xg, ndir * 4 * P, rk, lengths, y, ndir * P, h0, c0, h_last, c_last, B, T, P, ndir, dtype, ws, ws_bytes, None)


def test_the_state_entry_refuses_on_the_host():
    for dtype in (0, 1):
        # a state that can be taken: the answer is the shape's
        assert _lstm(dtype=dtype) == UNSUPPORTED
        assert _lstm(dtype=dtype, h_last=None, c_last=None) == UNSUPPORTED and _lstm(dtype=dtype, T=1 << 24) == UNSUPPORTED
        assert _lstm(dtype=dtype, h0=None, c0=None) == UNSUPPORTED  # no state: the stateless entry's answer
        # a backward direction cannot be continued
        assert _lstm(dtype=dtype, ndir=2) == INVALID
        assert _lstm(dtype=dtype, ndir=2, h0=None, c0=None) == UNSUPPORTED  # ... two directions without a state are the existing call
        # the new state in the old one's memory, in every pairing, whole and by one element at either end
        for kw in (dict(h_last=_at(H0)), dict(c_last=_at(C0)), dict(h_last=_at(C0)), dict(c_last=_at(H0)),
                   dict(h_last=_at(H0 + N - 8)), dict(h_last=_at(H0 - N + 8)), dict(c_last=_at(C0 + N - 8)), dict(c_last=_at(C0 - N + 8))):
            assert _lstm(dtype=dtype, **kw) == INVALID, kw
        # ... and right beside it is fine
        for kw in (dict(h_last=_at(H0 + N)), dict(h_last=_at(H0 - N)), dict(c_last=_at(C0 + N)), dict(c_last=_at(C0 - N))):
            assert _lstm(dtype=dtype, **kw) == UNSUPPORTED, kw
        # one half of a state alone
        assert _lstm(dtype=dtype, h0=None) == INVALID and _lstm(dtype=dtype, c0=None) == INVALID
        # alignment: h0 / c0 to 16 bytes, h_last / c_last to 8
        assert _lstm(dtype=dtype, h0=_at(H0 + 8)) == INVALID and _lstm(dtype=dtype, c0=_at(C0 + 4)) == INVALID
        assert _lstm(dtype=dtype, h0=_at(H0 + 16), c0=_at(C0 + 32)) == UNSUPPORTED
        assert _lstm(dtype=dtype, h_last=_at(HL + 4)) == INVALID and _lstm(dtype=dtype, c_last=_at(CL + 4)) == INVALID
        assert _lstm(dtype=dtype, h_last=_at(HL + 8), c_last=_at(CL + 8)) == UNSUPPORTED
    # what tfasr_lstm_infer_fwd refuses, this entry refuses too, with and without a state
    for kw in (dict(xg=None), dict(rk=None), dict(y=None), dict(ws=None), dict(B=0), dict(T=0), dict(P=0), dict(ndir=3), dict(dtype=2)):
        assert _lstm(**kw) == INVALID, kw
        assert _lstm(h0=None, c0=None, **kw) == INVALID, kw


def test_the_stateless_entry_answers_as_before():
    """nothing existing changes: the rules above belong to a call with a state"""
    one = "tfasr_lstm_infer_fwd"
    assert _lstm(entry=one) == UNSUPPORTED and _lstm(entry=one, ndir=2) == UNSUPPORTED
    assert _lstm(entry=one, h_last=_at(HL + 4), c_last=_at(CL + 4)) == UNSUPPORTED  # (4-byte aligned outputs were never refused)
    # a legal shape with a workspace one byte short ends at the workspace check, on both entries
    need = K.lstm_infer_workspace_size(2, 3, 32, 1, 1)
    assert need > 0
    assert _lstm(entry=one, B=2, T=3, P=32, ws_bytes=need - 1) == INVALID and _lstm(B=2, T=3, P=32, ws_bytes=need - 1) == INVALID


def _rowconv(x=f, state=f, w=f, scale=f, shift=f, nv=f, y=f, B=2, C=16, d=512, taps=5, dtype=0):
    return _lib.load().tfasr_stream_rowconv_fwd(x, state, w, scale, shift, nv, y, B, C, d, taps, dtype, None)


def test_rowconv_limits_and_arguments():
    assert _rowconv(C=K.STREAM_MAX_CHUNK + 1) == UNSUPPORTED
    assert _rowconv(taps=33) == UNSUPPORTED
    assert _rowconv(B=65536) == UNSUPPORTED
    for kw in (dict(x=None), dict(state=None), dict(w=None), dict(scale=None), dict(shift=None), dict(nv=None), dict(y=None), dict(B=0),
               dict(C=0), dict(d=0), dict(taps=0), dict(B=-1), dict(C=-4), dict(dtype=2), dict(dtype=-1)):
        assert _rowconv(**kw) == INVALID, kw
    # an argument that is wrong wins over a size that is merely too large
    assert _rowconv(C=K.STREAM_MAX_CHUNK + 1, y=None) == INVALID and _rowconv(taps=33, dtype=3) == INVALID


def test_model_surface():
    for name in ("stream", "stream_state", "encode_chunk"):
        assert callable(getattr(DeepSpeech2CTC, name)) and getattr(DeepSpeech2CTC, name) is not DeepSpeech2CTC._inference_only, name
    for name in ("train_step", "loss_and_backward", "compile"):
        assert getattr(DeepSpeech2CTC, name) is DeepSpeech2CTC._inference_only, name
    sig = lambda fn: [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
    assert sig(DeepSpeech2CTC.stream) == sig(JasperCTC.stream) == [("batch_size", 1), ("chunk_frames", 32), ("beam_width", 0),
                                                                   ("max_frames", 3000), ("precision", None)]
    assert sig(DeepSpeech2CTC.stream_state) == sig(JasperCTC.stream_state)
    assert all(callable(getattr(streaming.DS2StreamState, n)) for n in ("reset", "export", "load", "reference_states"))
    assert callable(streaming.ds2_encode_chunk)


class _M:  # check_streamable reads the config only
    def __init__(self, cfg):
        self.cfg = cfg


def test_check_streamable_on_deepspeech2_configs():
    streaming.check_streamable(_M(configs.deepspeech2(29, variant="uni")))
    streaming.check_streamable(_M(configs.deepspeech2_tiny(conv_padding="causal", rnn_bidirectional=False, rnn_rowconv=2)))
    streaming.check_streamable(_M(configs.deepspeech2_tiny(conv_padding="causal", rnn_bidirectional=False, rnn_rowconv=0)))
    refused = {
        "rnn_bidirectional": configs.deepspeech2(29),
        "conv_padding": configs.deepspeech2_tiny(conv_padding="same", rnn_bidirectional=False, rnn_rowconv=2),
    }
    for reason, cfg in refused.items():
        with pytest.raises(NotImplementedError, match="inference only, and this configuration cannot be streamed.*" + reason):
            streaming.check_streamable(_M(cfg))


def test_refusal_comes_before_any_argument_is_touched():
    m = object.__new__(DeepSpeech2CTC)
    m.cfg = configs.deepspeech2_tiny()  # "same" padding, bidirectional
    for call in (lambda: m.stream(), lambda: m.stream(batch_size=-5, beam_width=1000, chunk_frames=7), lambda: m.stream_state(),
                 lambda: m.stream_state(batch_size=None), lambda: m.encode_chunk(None, None, None)):
        with pytest.raises(NotImplementedError, match="inference only.*rnn_bidirectional"):
            call()
    for call in (lambda: m.train_step(None), lambda: m.loss_and_backward(None), lambda: m.compile()):
        with pytest.raises(NotImplementedError, match="inference only"):
            call()
