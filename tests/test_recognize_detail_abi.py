"""The detail variants of the greedy searches' entry points (tfasr_decode_update_detail, tfasr_decode_steps_detail,
tfasr_ctc_greedy_decode_detail; added under ABI 44): the symbols, the wrappers, the model surface and the host-side argument checks answer
without a GPU."""
import ctypes
import os
import re

import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

NEW = {"tfasr_decode_update_detail": 24, "tfasr_decode_steps_detail": 41, "tfasr_ctc_greedy_decode_detail": 16}
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
        assert callable(getattr(K, name[len("tfasr_"):])), name
    # the plain entry points keep their signatures: the detail variants add three buffers (the CTC one: five and the score)
    assert len(_lib.SIGNATURES["tfasr_decode_update"][1]) == NEW["tfasr_decode_update_detail"] - 3
    assert len(_lib.SIGNATURES["tfasr_decode_steps"][1]) == NEW["tfasr_decode_steps_detail"] - 3
    assert len(_lib.SIGNATURES["tfasr_ctc_greedy_decode"][1]) == NEW["tfasr_ctc_greedy_decode_detail"] - 5


def _update(logits=f, active=f, nframes=f, frame_idx=f, prev_tok=f, tok_idx=f, tokens=f, per_frame=f, h_new=f, c_new=f, h=f, c=f, tok_frames=f,
            tok_logp=f, tok_entropy=f, B=4, V=1000, P=320, mode=0, dtype=0):
    return _lib.load().tfasr_decode_update_detail(logits, active, nframes, frame_idx, prev_tok, tok_idx, tokens, per_frame, h_new, c_new, h, c,
                                                  tok_frames, tok_logp, tok_entropy, B, V, P, 48, 0, mode, 3, dtype, None)


def test_update_detail_refuses_bad_arguments_on_the_host():
    for name in ("logits", "active", "nframes", "frame_idx", "prev_tok", "tok_idx", "tokens", "h_new", "c_new", "h", "c", "tok_frames", "tok_logp",
                 "tok_entropy"):
        assert _update(**{name: None}) == INVALID, name
    for kw in (dict(B=0), dict(B=-1), dict(V=0), dict(P=0), dict(dtype=2), dict(mode=3), dict(mode=-1)):
        assert _update(**kw) == INVALID, kw
    assert _update(per_frame=None, mode=2) == INVALID
    assert _update(per_frame=None, mode=1, B=1) == INVALID and _update(mode=1, B=2) == INVALID  # (as tfasr_decode_update)


def _steps(tok_frames=f, tok_logp=f, tok_entropy=f, tokens=f, emb=f, B=4, V=1000, iters=4):
    return _lib.load().tfasr_decode_steps_detail(emb, f, f, f, f, f, f, f, f, f, None, f, f, f, f, f, f, f, f, f, f, f, f, tokens, f, tok_frames,
                                                 tok_logp, tok_entropy, B, 12, 320, 320, 320, V, 48, 0, 0, 3, 1e-3, iters, None)


def test_steps_detail_refuses_bad_arguments_on_the_host():
    for kw in (dict(tok_frames=None), dict(tok_logp=None), dict(tok_entropy=None), dict(tokens=None), dict(emb=None), dict(B=0), dict(B=65), dict(V=1),
               dict(iters=0), dict(iters=-3)):
        assert _steps(**kw) == INVALID, kw
    assert _steps(V=1004) == _lib.STATUS_UNSUPPORTED  # (V % 8: the per-op loop, as tfasr_decode_steps)


def _ctc(logits=f, logit_len=f, ws=f, tokens=f, tokens_len=f, starts=f, ends=f, tok_logp=f, tok_entropy=f, score=f, B=2, T=16, V=29, dtype=0):
    return _lib.load().tfasr_ctc_greedy_decode_detail(logits, logit_len, ws, tokens, tokens_len, starts, ends, tok_logp, tok_entropy, score, B, T, V,
                                                      0, dtype, None)


def test_ctc_detail_refuses_bad_arguments_on_the_host():
    for name in ("logits", "logit_len", "ws", "tokens", "tokens_len", "starts", "ends", "tok_logp", "tok_entropy", "score"):
        assert _ctc(**{name: None}) == INVALID, name
    for kw in (dict(B=0), dict(T=0), dict(V=0), dict(B=-2), dict(dtype=2)):
        assert _ctc(**kw) == INVALID, kw


def test_wrappers_refuse_cpu_tensors_and_misshapen_buffers():
    z = torch.zeros(2, 5)
    i = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(Exception):
        K.ctc_greedy_decode_detail(torch.zeros(2, 5, 7), i)
    tokens = torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(ValueError, match="detail buffers"):
        K.decode_update_detail(z, i, i, i, i, i, tokens, None, z, z, z, z, tokens.float(), z, z, 5, 0, 0, 3)
    with pytest.raises(ValueError, match="detail buffers"):
        K.decode_update_detail(z, i, i, i, i, i, tokens, None, z, z, z, z, tokens, z[:, :4], z, 5, 0, 0, 3)


def test_model_surface_without_a_gpu():
    from tensorflowasr_amd import schemas
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.contextnet import ContextNetTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC
    from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC
    from tensorflowasr_amd.jasper import JasperCTC
    from tensorflowasr_amd.rnnt import RnnTransducer
    from tensorflowasr_amd.transformer import TransformerCTC, TransformerTransducer

    for cls in (ConformerTransducer, ContextNetTransducer, TransformerTransducer, RnnTransducer):
        assert cls.recognize_detailed is ConformerTransducer.recognize_detailed
        assert cls.recognize_encoded_detailed is ConformerTransducer.recognize_encoded_detailed
    for cls in (ConformerCTC, TransformerCTC, JasperCTC, DeepSpeech2CTC):
        assert cls.recognize_detailed is ConformerCTC.recognize_detailed
        with pytest.raises(NotImplementedError, match="CTC"):
            cls.recognize_encoded_detailed(object.__new__(cls))
    assert schemas.RecognizeOutput._fields[:3] == ("predict", "frames", "ends")
    assert callable(schemas.token_confidences) and callable(schemas.word_details)
