"""LM shallow fusion, the surface that answers without a GPU: the three tfasr_ctc_beam_search_lm* symbols and tfasr_ngram_lm_t are
declared and exported under ABI 44, every argument check happens on the host before any launch, evaluate has its appended keywords
and the CTC model classes their two methods."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ctc_lm_oracle as O
from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tfasr_ctc_beam_search_lm_host", "tfasr_ctc_beam_search_lm_workspace_size", "tfasr_ctc_beam_search_lm")


def test_symbols_declared_and_exported_under_abi_44():
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "tfasr_hip.h")).read()
    assert re.search(r"#define\s+TFASR_ABI_VERSION\s+44\b", hdr)
    assert _lib.ABI_VERSION == 44 and lib.tfasr_abi_version() == 44
    for name in NAMES:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr), name
        assert getattr(lib, name) is not None
    assert len(_lib.SIGNATURES["tfasr_ctc_beam_search_lm_host"][1]) == 14
    assert len(_lib.SIGNATURES["tfasr_ctc_beam_search_lm_workspace_size"][1]) == 5
    assert len(_lib.SIGNATURES["tfasr_ctc_beam_search_lm"][1]) == 18
    assert "tfasr_ngram_lm_t" in hdr and re.search(r"#define\s+TFASR_CTC_LM_MAX_BEAM\s+32\b", hdr) and K.CTC_LM_MAX_BEAM == 32


def test_struct_size_matches_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tfasr_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", '
                   'sizeof(tfasr_ngram_lm_t), offsetof(tfasr_ngram_lm_t, depth), offsetof(tfasr_ngram_lm_t, eos)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = K.NGramLmStruct
    assert sizes == [ctypes.sizeof(S), S.depth.offset, S.eos.offset]


def _ws(B, T, V, W):
    n = ctypes.c_size_t(0)
    st = _lib.load().tfasr_ctc_beam_search_lm_workspace_size(B, T, V, W, ctypes.byref(n))
    return st, n.value


def _plain_ws(B, T, V, W):
    n = ctypes.c_size_t(0)
    assert _lib.load().tfasr_ctc_beam_search_workspace_size(B, T, V, W, ctypes.byref(n)) == 0
    return n.value


def test_workspace_size():
    st, n = _ws(4, 50, 29, 4)
    assert st == 0 and n >= _plain_ws(4, 50, 29, 4) + 2 * 4 * (1 + 4 * 50) * 4  # the plain search's, plus two arrays per trie node
    assert _ws(4, 50, 29, 32)[0] == 0
    assert _ws(4, 50, 29, 33)[0] == _lib.STATUS_UNSUPPORTED
    for args in ((0, 10, 5, 2), (2, 0, 5, 2), (2, 10, 1, 2), (2, 10, 5, 0)):
        assert _ws(*args)[0] == 1, args
    assert _lib.load().tfasr_ctc_beam_search_lm_workspace_size(2, 10, 5, 2, None) != 0


def _tables(**over):
    t = O.markov_lm(5, 0, 2, seed=1).tables(0.5, 0.0)
    st = K.NGramLmStruct(*[getattr(t, a).ctypes.data for a in K._LM_ARRAYS], t.nodes, t.table_size, t.order, t.start, t.eos)
    for k, v in over.items():
        setattr(st, k, v)
    return t, st


def test_device_entry_refuses_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every check below happens on the host before any launch
    B, T, V = 2, 10, 5
    _, need = _ws(B, T, V, 4)
    keep, good = _tables()

    def call(logits=fake, llen=fake, W=4, P=1, blank=0, dtype=0, lm=good, toks=fake, tlen=fake, sc=fake, lp=fake, ls=fake, ws=fake, wsb=need,
             V_=V):
        lmp = None if lm is None else ctypes.addressof(lm)
        return lib.tfasr_ctc_beam_search_lm(logits, llen, B, T, V_, W, P, blank, dtype, lmp, toks, tlen, sc, lp, ls, ws, wsb, None)

    for kw in ("logits", "llen", "lm", "toks", "tlen", "sc", "lp", "ls", "ws"):
        assert call(**{kw: None}) == 1, kw
    assert call(W=33) == _lib.STATUS_UNSUPPORTED and call(W=64) == _lib.STATUS_UNSUPPORTED
    assert call(W=0) == 1 and call(W=65) == 1
    assert call(P=0) == 1 and call(P=5) == 1
    assert call(blank=-1) == 1 and call(blank=V) == 1
    assert call(V_=1, blank=0) == 1
    assert call(dtype=7) == 1
    assert call(wsb=need - 1) == 1
    for bad in (dict(table_size=keep.table_size - 1), dict(table_size=0), dict(order=0), dict(nodes=0), dict(start=keep.nodes), dict(eos=-2),
                dict(keys=None), dict(vals=None), dict(wlogp=None), dict(wbow=None), dict(weos=None), dict(suffix=None), dict(depth=None)):
        assert call(lm=_tables(**bad)[1]) == 1, bad


def test_host_entry_refuses_bad_arguments():
    lib = _lib.load()
    B, T, V = 2, 6, 5
    x = np.zeros((B, T, V), np.float32)
    ln = np.array([6, 3], np.int32)
    toks, n = np.zeros((B, 4, T), np.int32), np.zeros((B, 4), np.int32)
    sc, lp, ls = (np.zeros((B, 4), np.float32) for _ in range(3))
    keep, good = _tables()

    def call(logits=x, llen=ln, W=4, P=1, blank=0, lm=good, toks_=toks, n_=n, sc_=sc, lp_=lp, ls_=ls, V_=V):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        lmp = None if lm is None else ctypes.addressof(lm)
        return lib.tfasr_ctc_beam_search_lm_host(p(logits), p(llen), B, T, V_, W, P, blank, lmp, p(toks_), p(n_), p(sc_), p(lp_), p(ls_))

    assert call() == 0
    for kw in ("logits", "llen", "lm", "toks_", "n_", "sc_", "lp_", "ls_"):
        assert call(**{kw: None}) == 1, kw
    assert call(W=33) == _lib.STATUS_UNSUPPORTED
    assert call(W=0) == 1 and call(P=0) == 1 and call(P=5) == 1 and call(blank=-1) == 1 and call(blank=V) == 1 and call(V_=1) == 1
    for bad in (dict(table_size=keep.table_size + 2), dict(order=0), dict(order=-1)):
        assert call(lm=_tables(**bad)[1]) == 1, bad


@pytest.mark.parametrize("kw", [dict(beam_width=0), dict(beam_width=33), dict(beam_width=4, top_paths=5), dict(top_paths=0),
                                dict(blank_index=-1), dict(blank_index=5)])
def test_python_entries_raise_value_error(kw):
    tables = O.markov_lm(5, 0, 2, seed=1).tables(0.5, 0.0)
    logits, ln = torch.zeros(2, 10, 5), torch.tensor([10, 3], dtype=torch.int32)
    for fn in (K.ctc_beam_search_lm, K.ctc_beam_search_lm_host):
        with pytest.raises(ValueError) as e:
            fn(logits, ln, tables, **kw)
        if kw.get("beam_width") == 33:
            assert "32" in str(e.value)


def test_an_lm_of_another_vocabulary_or_blank_is_refused():
    """a smaller vocabulary would score <s> / </s> as classes, another blank would find no unigram: errors, not silent scores"""
    logits, ln = torch.zeros(2, 10, 5), torch.tensor([10, 3], dtype=torch.int32)
    small = O.markov_lm(4, 0, 2, seed=1).tables(0.5, 0.0)
    other_blank = O.markov_lm(5, 4, 2, seed=1).tables(0.5, 0.0)
    assert (small.vocab_size, small.blank, other_blank.vocab_size, other_blank.blank) == (4, 0, 5, 4)
    for fn in (K.ctc_beam_search_lm, K.ctc_beam_search_lm_host):
        with pytest.raises(ValueError, match="vocab_size 4"):
            fn(logits, ln, small, blank_index=0)
        with pytest.raises(ValueError, match="blank 4"):
            fn(logits, ln, other_blank, blank_index=0)
    assert len(K.ctc_beam_search_lm_host(logits, ln, other_blank, blank_index=4)) == 5

    from tensorflowasr_amd.ctc_model import ConformerCTC

    class Cfg:
        vocab_size = 5

    m = ConformerCTC.__new__(ConformerCTC)
    m.cfg, m.blank = Cfg, 0
    for name in ("recognize_beam_lm", "recognize_nbest_lm"):
        for lm in (O.markov_lm(4, 0, 2, seed=1), O.markov_lm(5, 4, 2, seed=1)):
            with pytest.raises(ValueError, match="language model"):
                getattr(m, name)(None, lm)


def test_evaluate_keywords_are_appended_with_their_defaults():
    from tensorflowasr_amd.base_model import BaseModel

    ps = list(inspect.signature(BaseModel.evaluate).parameters.values())
    assert [p.name for p in ps[-4:]] == ["batch_size", "lm", "lm_alpha", "lm_beta"]
    assert [p.default for p in ps[-3:]] == [None, 0.5, 0.0]


def test_ctc_classes_have_the_methods_and_transducers_do_not():
    from tensorflowasr_amd.conformer import ConformerTransducer
    from tensorflowasr_amd.ctc_model import ConformerCTC
    from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC
    from tensorflowasr_amd.jasper import JasperCTC
    from tensorflowasr_amd.transformer import TransformerCTC

    for cls in (ConformerCTC, TransformerCTC, JasperCTC, DeepSpeech2CTC):
        for name, args in (("recognize_beam_lm", ["inputs", "lm", "beam_width", "alpha", "beta", "device_search"]),
                           ("recognize_nbest_lm", ["inputs", "lm", "beam_width", "top_paths", "alpha", "beta"])):
            sig = inspect.signature(getattr(cls, name))
            assert list(sig.parameters)[1:] == args, (cls, name)
            assert "self.blank" in getattr(cls, name).__doc__
    assert not hasattr(ConformerTransducer, "recognize_beam_lm") and not hasattr(ConformerTransducer, "recognize_nbest_lm")
