"""Streaming entry points (csrc/stream.hip, tfasr_logmel_stream, tfasr_ctc_greedy_decode_carry, mode 2 of the greedy search; added
under ABI 44): the symbols, the limits and the host-side argument checks answer without a GPU."""
import ctypes
import os
import re

import pytest

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

NEW = {"tfasr_stream_attn_fwd": 17, "tfasr_stream_kv_append": 12, "tfasr_stream_glu_dwconv_fwd": 12, "tfasr_logmel_stream": 19,
       "tfasr_ctc_greedy_decode_carry": 12}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
MAX_CHUNK, MAX_KEYS, MAX_HEAD = 32, 512, 128
INVALID, UNSUPPORTED = 1, _lib.STATUS_UNSUPPORTED
f = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch


def test_symbols_declared_exported_and_abi_unchanged():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    src = open(HEADER).read()
    for name, nargs in NEW.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    for name, val in (("CHUNK", MAX_CHUNK), ("KEYS", MAX_KEYS), ("HEAD", MAX_HEAD)):
        assert re.search(rf"#define TFASR_STREAM_MAX_{name} {val}\b", src), name
    assert (K.STREAM_MAX_CHUNK, K.STREAM_MAX_KEYS, K.STREAM_MAX_HEAD) == (MAX_CHUNK, MAX_KEYS, MAX_HEAD)
    assert "#define TFASR_ABI_VERSION 44" in src


def _attn(qkv=f, u=f, v=f, pos=f, kc=f, vc=f, seen=f, nv=f, out=f, B=2, C=16, H=4, dh=64, hist=64, dtype=0):
    return _lib.load().tfasr_stream_attn_fwd(qkv, u, v, pos, kc, vc, seen, nv, out, B, C, H, dh, hist, 0.125, dtype, None)


def test_attention_limits_and_arguments():
    assert _attn(C=MAX_CHUNK + 1) == UNSUPPORTED
    assert _attn(C=16, hist=MAX_KEYS - 15) == UNSUPPORTED
    assert _attn(dh=MAX_HEAD + 8) == UNSUPPORTED
    for kw in (dict(qkv=None), dict(u=None), dict(v=None), dict(pos=None), dict(kc=None), dict(vc=None), dict(seen=None), dict(nv=None),
               dict(out=None), dict(B=0), dict(C=0), dict(H=0), dict(dh=0), dict(hist=-1), dict(dtype=2)):
        assert _attn(**kw) == INVALID, kw


def test_ring_append_limits_and_arguments():
    lib = _lib.load()

    def call(qkv=f, kc=f, vc=f, seen=f, nv=f, B=2, C=16, H=4, dh=64, hist=64, dtype=0):
        return lib.tfasr_stream_kv_append(qkv, kc, vc, seen, nv, B, C, H, dh, hist, dtype, None)

    assert call(C=MAX_CHUNK + 1) == UNSUPPORTED and call(hist=MAX_KEYS) == UNSUPPORTED
    for kw in (dict(qkv=None), dict(kc=None), dict(vc=None), dict(seen=None), dict(nv=None), dict(B=0), dict(C=-1), dict(H=0), dict(dh=0),
               dict(hist=-2), dict(dtype=5)):
        assert call(**kw) == INVALID, kw
    assert call(kc=None, vc=None, hist=0) == 0  # no ring: nothing to launch


def test_glu_dwconv_limits_and_arguments():
    lib = _lib.load()

    def call(a=f, st=f, w=f, b=f, nv=f, y=f, B=2, C=16, d=144, Kk=31, dtype=0):
        return lib.tfasr_stream_glu_dwconv_fwd(a, st, w, b, nv, y, B, C, d, Kk, dtype, None)

    assert call(C=MAX_CHUNK + 1) == UNSUPPORTED and call(Kk=33) == UNSUPPORTED
    for kw in (dict(a=None), dict(st=None), dict(w=None), dict(nv=None), dict(y=None), dict(B=0), dict(C=0), dict(d=0), dict(Kk=0), dict(dtype=2)):
        assert call(**kw) == INVALID, kw


def test_logmel_stream_arguments():
    lib = _lib.load()

    def call(sig=f, nlen=f, prev=f, hp=f, B=2, N=10480, win=f, fl=400, fs=160, nfft=512, melw=f, band=f, F=80, out=f, T0=64, dtype=0):
        return lib.tfasr_logmel_stream(sig, nlen, prev, hp, B, N, 0.97, win, fl, fs, nfft, melw, band, F, 1e-6, out, T0, dtype, None)

    for kw in (dict(sig=None), dict(nlen=None), dict(prev=None), dict(hp=None), dict(win=None), dict(melw=None), dict(band=None), dict(out=None),
               dict(B=0), dict(N=0), dict(F=0), dict(T0=0), dict(dtype=3)):
        assert call(**kw) == INVALID, kw
    assert call(nfft=1024) == UNSUPPORTED and call(fl=600) == UNSUPPORTED


def test_search_mode_2_needs_its_counter_and_ctc_carry_its_class():
    lib = _lib.load()

    def update(per_frame, mode, B=4):
        return lib.tfasr_decode_update(f, f, f, f, f, f, f, per_frame, f, f, f, f, B, 1000, 320, 48, 0, mode, 3, 0, None)

    assert update(None, 2) == INVALID
    assert update(None, 1, B=1) == INVALID and update(f, 1, B=2) == INVALID  # (modes 0 / 1: as before)
    assert lib.tfasr_ctc_greedy_decode_carry(f, f, None, f, f, f, 2, 16, 29, 0, 0, None) == INVALID
    assert lib.tfasr_ctc_greedy_decode_carry(f, f, f, f, f, f, 0, 16, 29, 0, 0, None) == INVALID


def test_model_surface_and_refusals_without_a_gpu():
    from tensorflowasr_amd import configs, schemas, streaming
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.contextnet import ContextNetTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC

    for cls in (ConformerTransducer, ConformerCTC):
        assert callable(cls.stream) and callable(cls.stream_state) and callable(cls.encode_chunk)
    with pytest.raises(NotImplementedError, match="squeeze-and-excite"):
        ContextNetTransducer.stream(object.__new__(ContextNetTransducer))
    assert streaming.StreamOutput._fields == ("tokens", "tokens_length", "frames")
    assert "previous_encoder_states" in schemas.PredictInput._fields and "next_encoder_states" in schemas.PredictOutput._fields

    class _M:  # check_streamable reads the config and the stored head size only
        def __init__(self, **over):
            self.cfg = configs.conformer_tiny(**over)
            self.ps = type("P", (), dict(head_phys=self.cfg.head_size))()

    with pytest.raises(ValueError, match="chunk_size is None"):
        streaming.check_streamable(_M())
    with pytest.raises(ValueError, match="unlimited history"):
        streaming.check_streamable(_M(chunk_size=2, history_size=-1))
    with pytest.raises(ValueError, match="limits"):
        streaming.check_streamable(_M(chunk_size=MAX_CHUNK + 1, history_size=4))
    with pytest.raises(ValueError, match="limits"):
        streaming.check_streamable(_M(chunk_size=16, history_size=MAX_KEYS))
    streaming.check_streamable(_M(chunk_size=16, history_size=64))
