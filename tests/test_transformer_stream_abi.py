"""The streaming Transformer's entry points (tfasr_stream_attn_plain_fwd, tfasr_stream_add_pe; added under ABI 44): the symbols, the
host-side argument checks, the model surface and check_streamable's Transformer branch answer without a GPU."""
import ctypes
import os
import re

import pytest

from tensorflowasr_amd import _lib, configs, streaming
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.transformer import TransformerCTC, TransformerTransducer

NEW = {"tfasr_stream_attn_plain_fwd": 15, "tfasr_stream_add_pe": 11}
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
MAX_CHUNK, MAX_KEYS, MAX_HEAD = 32, 512, 128
INVALID, UNSUPPORTED = 1, _lib.STATUS_UNSUPPORTED
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
    assert callable(K.stream_attn_plain_fwd) and callable(K.stream_add_pe)
    assert (K.STREAM_MAX_CHUNK, K.STREAM_MAX_KEYS, K.STREAM_MAX_HEAD) == (MAX_CHUNK, MAX_KEYS, MAX_HEAD)


def _attn(qkv=f, kc=f, vc=f, seen=f, nv=f, out=f, B=2, C=16, H=4, dh=128, hist=64, causal=0, dtype=0):
    return _lib.load().tfasr_stream_attn_plain_fwd(qkv, kc, vc, seen, nv, out, B, C, H, dh, hist, 0.125, causal, dtype, None)


def test_plain_attention_limits_and_arguments():
    assert _attn(C=MAX_CHUNK + 1) == UNSUPPORTED
    assert _attn(C=16, hist=MAX_KEYS - 15) == UNSUPPORTED
    assert _attn(dh=MAX_HEAD + 8) == UNSUPPORTED
    assert _attn(B=65536) == UNSUPPORTED
    for kw in (dict(qkv=None), dict(kc=None), dict(vc=None), dict(seen=None), dict(nv=None), dict(out=None), dict(B=0), dict(C=0), dict(H=0),
               dict(dh=0), dict(B=-1), dict(C=-2), dict(H=-1), dict(dh=-8), dict(hist=-1), dict(dtype=2), dict(dtype=-1)):
        assert _attn(**kw) == INVALID, kw
    # an argument that is wrong wins over a size that is merely too large
    assert _attn(C=MAX_CHUNK + 1, out=None) == INVALID and _attn(dh=MAX_HEAD + 8, dtype=3) == INVALID


def test_position_rows_arguments():
    lib = _lib.load()

    def call(x=f, pe=f, seen=f, nv=f, y=f, B=2, C=16, d=512, Tcap=256, dtype=0):
        return lib.tfasr_stream_add_pe(x, pe, seen, nv, y, B, C, d, Tcap, dtype, None)

    for kw in (dict(x=None), dict(pe=None), dict(seen=None), dict(nv=None), dict(y=None), dict(B=0), dict(C=0), dict(d=0), dict(Tcap=0),
               dict(B=-3), dict(Tcap=-1), dict(dtype=2)):
        assert call(**kw) == INVALID, kw


def test_model_surface():
    for cls in (TransformerCTC, TransformerTransducer):
        for name in ("stream", "stream_state", "encode_chunk"):
            assert callable(getattr(cls, name)) and getattr(cls, name) is not cls._inference_only, (cls.__name__, name)
        for name in ("train_step", "loss_and_backward", "compile"):
            assert getattr(cls, name) is cls._inference_only, (cls.__name__, name)
    import inspect

    sig = inspect.signature(TransformerCTC.stream)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("batch_size", 1), ("precision", None), ("max_tokens_per_frame", 3), ("beam_width", 0), ("max_frames", 3000)]
    for cls in (streaming.TransformerStreamState,):
        assert all(callable(getattr(cls, n)) for n in ("reset", "export", "load"))
    assert callable(streaming.transformer_encode_chunk)


class _T:  # check_streamable reads the config only
    def __init__(self, cfg):
        self.cfg = cfg


def test_check_streamable_on_transformer_configs():
    streaming.check_streamable(_T(configs.transformer(streaming=True)))  # the shipped base-streaming config: chunk 16, history 64
    streaming.check_streamable(_T(configs.transformer(streaming=True, use_attention_causal_mask=True)))  # the causal flag goes to the kernel
    streaming.check_streamable(_T(configs.transformer_tiny(chunk_size=4, history_size=0)))
    streaming.check_streamable(_T(configs.transformer(chunk_size=MAX_CHUNK, history_size=MAX_KEYS - MAX_CHUNK)))
    refused = {
        "chunk_size is None": configs.transformer(),
        "use_attention_auto_mask": configs.transformer(streaming=True, use_attention_auto_mask=False),
        "unlimited history": configs.transformer(chunk_size=16, history_size=-1),
        "limits": configs.transformer(chunk_size=MAX_CHUNK + 1, history_size=4),
    }
    for reason, cfg in refused.items():
        with pytest.raises(NotImplementedError, match="inference only.*" + reason):
            streaming.check_streamable(_T(cfg))
    with pytest.raises(NotImplementedError, match="inference only.*limits"):
        streaming.check_streamable(_T(configs.transformer(chunk_size=16, history_size=MAX_KEYS)))


def test_refusal_comes_before_any_argument_is_touched():
    """the three entry points of a model that cannot be streamed refuse whatever they are given (no device, no weights are needed)"""
    for cls, head in ((TransformerCTC, "ctc"), (TransformerTransducer, "rnnt")):
        m = object.__new__(cls)
        m.cfg = configs.transformer_tiny(head=head)  # full context
        for call in (lambda: m.stream(), lambda: m.stream(batch_size=-5, beam_width=1000), lambda: m.stream_state(),
                     lambda: m.stream_state(batch_size=None), lambda: m.encode_chunk(None, None, None)):
            with pytest.raises(NotImplementedError, match="inference only.*chunk_size is None"):
                call()


def test_conformer_and_jasper_configs_behave_as_before():
    class _M:
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
    streaming.check_streamable(type("J", (), dict(cfg=type("C", (), dict(encoder="jasper"))()))())
