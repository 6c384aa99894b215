"""The fused CTC beam search in pieces, the surface that answers without a GPU: the seven tfasr_ctc_beam_lm_* symbols are declared
and exported under ABI 44, the workspace is the plain stream's plus two arrays per trie node, a beam wider than 32 is UNSUPPORTED in
every entry, and every other bad argument is INVALID_VALUE - all from host-side checks, before any launch (the pointers handed over
here are never dereferenced)."""
import ctypes
import inspect
import os
import re

import pytest

import ctc_lm_oracle as O
from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {"tfasr_ctc_beam_lm_stream_workspace_size": 6, "tfasr_ctc_beam_lm_reset": 10, "tfasr_ctc_beam_lm_advance": 15,
         "tfasr_ctc_beam_lm_commit": 14, "tfasr_ctc_beam_lm_commit_horizon": 16, "tfasr_ctc_beam_lm_compact": 13,
         "tfasr_ctc_beam_lm_nbest": 17}
B, C, TCAP, V, W = 2, 4, 10, 5, 4
FAKE = ctypes.c_void_p(0x1000)
INVALID, UNSUPPORTED = 1, _lib.STATUS_UNSUPPORTED


def test_symbols_declared_and_exported_under_abi_44():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "tfasr_hip.h")).read()
    assert re.search(r"#define\s+TFASR_ABI_VERSION\s+44\b", hdr)
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    for name, n in NARGS.items():
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(lib, name) is not None
        assert len(_lib.SIGNATURES[name][1]) == n, name
    assert "THE SAME tables" in hdr  # the session rule is stated where the entries are declared


def _ws(name, *dims):
    n = ctypes.c_size_t(0)
    st = getattr(_lib.load(), name)(*dims, ctypes.byref(n))
    return st, n.value


def test_workspace_size():
    st, n = _ws("tfasr_ctc_beam_lm_stream_workspace_size", B, C, TCAP, V, W)
    pst, plain = _ws("tfasr_ctc_beam_stream_workspace_size", B, C, TCAP, V, W)
    assert st == 0 and pst == 0 and n >= plain + 2 * B * (1 + W * TCAP) * 4
    assert _ws("tfasr_ctc_beam_lm_stream_workspace_size", B, C, TCAP, 40, 32)[0] == 0
    assert _ws("tfasr_ctc_beam_lm_stream_workspace_size", B, C, TCAP, 40, 33)[0] == UNSUPPORTED
    for dims in ((0, C, TCAP, V, W), (B, 0, TCAP, V, W), (B, TCAP + 1, TCAP, V, W), (B, C, 0, V, W), (B, C, TCAP, 1, W), (B, C, TCAP, V, 0),
                 (B, C, TCAP, V, 65)):
        assert _ws("tfasr_ctc_beam_lm_stream_workspace_size", *dims)[0] == INVALID, dims
    assert _lib.load().tfasr_ctc_beam_lm_stream_workspace_size(B, C, TCAP, V, W, None) == INVALID


def _tables(**over):
    t = O.markov_lm(V, 0, 2, seed=1).tables(0.5, 0.0)
    st = K.NGramLmStruct(*[getattr(t, a).ctypes.data for a in K._LM_ARRAYS], t.nodes, t.table_size, t.order, t.start, t.eos)
    for k, v in over.items():
        setattr(st, k, v)
    return t, st


KEEP, GOOD = _tables()
NEED = _ws("tfasr_ctc_beam_lm_stream_workspace_size", B, C, TCAP, V, W)[1]


def _lmp(lm):
    return None if lm is None else ctypes.addressof(lm)


def reset(mask=None, W_=W, lm=GOOD, ws=FAKE, wsb=NEED, C_=C):
    return _lib.load().tfasr_ctc_beam_lm_reset(mask, B, C_, TCAP, V, W_, _lmp(lm), ws, wsb, None)


def advance(logits=FAKE, nvalid=FAKE, W_=W, Cn=C, blank=0, dtype=0, after=TCAP, lm=GOOD, ws=FAKE, wsb=NEED):
    return _lib.load().tfasr_ctc_beam_lm_advance(logits, nvalid, B, C, Cn, TCAP, V, W_, blank, dtype, after, _lmp(lm), ws, wsb, None)


def commit(fin=None, committed=FAKE, toks=FAKE, ntoks=FAKE, W_=W, width=TCAP, lm=GOOD, ws=FAKE, wsb=NEED):
    return _lib.load().tfasr_ctc_beam_lm_commit(fin, committed, toks, ntoks, B, C, TCAP, V, W_, width, _lmp(lm), ws, wsb, None)


def commit_horizon(fin=None, committed=FAKE, toks=FAKE, ntoks=FAKE, hstate=FAKE, H=8, W_=W, width=TCAP, lm=GOOD, ws=FAKE, wsb=NEED):
    return _lib.load().tfasr_ctc_beam_lm_commit_horizon(fin, committed, toks, ntoks, hstate, H, B, C, TCAP, V, W_, width, _lmp(lm), ws, wsb,
                                                        None)


def compact(mask=FAKE, committed=FAKE, hstate=FAKE, H=8, out=FAKE, W_=W, ws=FAKE, wsb=NEED):
    return _lib.load().tfasr_ctc_beam_lm_compact(mask, committed, hstate, H, out, B, C, TCAP, V, W_, ws, wsb, None)


def nbest(fin=None, W_=W, P=2, width=TCAP, toks=FAKE, tlen=FAKE, sc=FAKE, lp=FAKE, ls=FAKE, lm=GOOD, ws=FAKE, wsb=NEED):
    return _lib.load().tfasr_ctc_beam_lm_nbest(fin, B, C, TCAP, V, W_, P, width, toks, tlen, sc, lp, ls, _lmp(lm), ws, wsb, None)


ENTRIES = (reset, advance, commit, commit_horizon, compact, nbest)


@pytest.mark.parametrize("fn", ENTRIES, ids=lambda f: f.__name__)
def test_a_beam_wider_than_32_is_unsupported_before_any_launch(fn):
    big = 1 << 40  # (a workspace of any size: the width is refused first)
    assert fn(W_=33, wsb=big) == UNSUPPORTED and fn(W_=64, wsb=big) == UNSUPPORTED
    assert fn(W_=0) == INVALID and fn(W_=65) == INVALID


@pytest.mark.parametrize("fn", ENTRIES, ids=lambda f: f.__name__)
def test_null_pointers_and_a_short_workspace_are_invalid(fn):
    optional = {"mask": reset, "fin": None, "hstate": compact}  # NULL allowed: reset's mask, every final_mask, compact's horizon state
    for name, p in inspect.signature(fn).parameters.items():
        if p.default is FAKE and optional.get(name, 0) is not fn:
            assert fn(**{name: None}) == INVALID, name
    if fn is not compact:
        assert fn(lm=None) == INVALID
    assert fn(wsb=NEED - 1) == INVALID and fn(wsb=0) == INVALID


@pytest.mark.parametrize("fn", [f for f in ENTRIES if f is not compact], ids=lambda f: f.__name__)
def test_a_bad_table_struct_is_invalid(fn):
    for bad in (dict(table_size=KEEP.table_size - 1), dict(table_size=0), dict(order=0), dict(nodes=0), dict(start=KEEP.nodes), dict(eos=-2),
                dict(keys=None), dict(vals=None), dict(wlogp=None), dict(wbow=None), dict(weos=None), dict(suffix=None), dict(depth=None)):
        assert fn(lm=_tables(**bad)[1]) == INVALID, bad


def test_the_other_argument_checks():
    assert advance(Cn=C + 1) == INVALID and advance(Cn=0) == INVALID
    assert advance(after=TCAP + 1) == INVALID and advance(after=-1) == INVALID
    assert advance(blank=-1) == INVALID and advance(blank=V) == INVALID and advance(dtype=7) == INVALID
    assert nbest(P=W + 1) == INVALID and nbest(P=0) == INVALID
    assert nbest(width=0) == INVALID and nbest(width=TCAP + 1) == INVALID
    assert commit(width=0) == INVALID and commit_horizon(width=0) == INVALID
    assert commit_horizon(H=0) == INVALID and commit_horizon(H=4097) == INVALID
    assert compact(H=0) == INVALID and compact(hstate=None, H=8) == INVALID
    assert reset(C_=TCAP + 1) == INVALID


def test_the_python_class_checks_before_any_device_work():
    t = O.markov_lm(V, 0, 2, seed=1).tables(0.5, 0.0)
    with pytest.raises(ValueError, match="32"):
        K.CtcLmBeamStream(B, C, TCAP, V, 33, t, blank_index=0, device="cpu")
    with pytest.raises(ValueError, match="blank"):
        K.CtcLmBeamStream(B, C, TCAP, V, W, t, blank_index=V - 1, device="cpu")  # the tables were built for blank 0
    with pytest.raises(ValueError, match="chunk capacity"):
        K.CtcLmBeamStream(B, TCAP + 1, TCAP, V, W, t, blank_index=0, device="cpu")
    assert list(inspect.signature(K.CtcLmBeamStream.nbest).parameters)[1:] == ["top_paths", "final_rows"]


def test_the_sessions_take_the_lm_keywords_and_refuse_without_a_device():
    from tensorflowasr_amd import streaming
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC
    from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC
    from tensorflowasr_amd.jasper import JasperCTC
    from tensorflowasr_amd.transformer import TransformerCTC

    for cls in (ConformerCTC, TransformerCTC, JasperCTC, DeepSpeech2CTC, ConformerTransducer):
        assert cls.stream_lm is ConformerCTC.stream_lm  # one door, the arguments of the class's own stream() (whose signature is pinned)
        assert "lm" not in inspect.signature(cls.stream).parameters
    ps = list(inspect.signature(ConformerCTC.stream_lm).parameters.values())
    assert [(p.name, p.default) for p in ps[-3:-1]] == [("lm_alpha", 0.5), ("lm_beta", 0.0)] and ps[1].name == "lm"
    assert "self.blank" in ConformerCTC.stream_lm.__doc__ and callable(streaming.StreamingRecognizer.with_lm)
    assert callable(streaming.StreamingRecognizer.hypotheses_lm)
    assert "self.blank" in streaming.StreamingRecognizer.__doc__ and "V-1" in streaming.StreamingRecognizer.__doc__

    class Cfg:
        vocab_size, head = V, "ctc"

    m = ConformerCTC.__new__(ConformerCTC)
    m.cfg, m.blank = Cfg, 0
    lm = O.markov_lm(V, 0, 2, seed=1)
    assert streaming.check_stream_lm(m, None, 0.5, 0.0, 0) is None
    assert streaming.check_stream_lm(m, lm, 0.5, 0.0, 4) is lm.tables(0.5, 0.0)
    with pytest.raises(ValueError, match="beam_width >= 1"):
        streaming.check_stream_lm(m, lm, 0.5, 0.0, 0)
    with pytest.raises(ValueError, match="32"):
        streaming.check_stream_lm(m, lm, 0.5, 0.0, 33)
    with pytest.raises(ValueError, match="detail"):
        streaming.check_stream_lm(m, lm, 0.5, 0.0, 4, detail=True)
    with pytest.raises(ValueError, match="language model"):
        streaming.check_stream_lm(m, O.markov_lm(V - 1, 0, 2, seed=1), 0.5, 0.0, 4)

    class TCfg:
        vocab_size, head = V, "transducer"

    t = ConformerTransducer.__new__(ConformerTransducer)
    t.cfg, t.blank = TCfg, 0
    with pytest.raises(NotImplementedError, match="prediction network is its LM"):
        streaming.check_stream_lm(t, lm, 0.5, 0.0, 4)
    # the door judges its arguments before it opens the session (these objects could not open one)
    with pytest.raises(NotImplementedError, match="prediction network is its LM"):
        t.stream_lm(lm, 1, beam_width=4)
    with pytest.raises(ValueError, match="beam_width >= 1"):
        m.stream_lm(lm, 1)
    with pytest.raises(ValueError, match="32"):
        m.stream_lm(lm, 1, beam_width=33)
    with pytest.raises(ValueError, match="32"):
        m.stream_horizon(8, 1, beam_width=33, lm=lm)
