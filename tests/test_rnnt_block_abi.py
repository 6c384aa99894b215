"""tfasr_rnnt_block_tail_fwd (the RnnTransducerBlock's LayerNorm + Dense tail; declaration added under ABI 44, nothing existing changes):
the symbol, its ctypes signature, and the answers the library gives on the host before any launch.  Nothing here needs a GPU.

The ABI number stays 44: the entry is a declaration only, and the version is pinned by the ABI tests of every earlier addition
(symbols-only additions never moved it: INTEGRATION.md); `_lib.load()` refuses a library that lacks a declared symbol."""
import ctypes
import inspect
import os
import re

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

NAME, NARGS = "tfasr_rnnt_block_tail_fwd", 19
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tfasr_hip.h")
INVALID, UNSUPPORTED = 1, _lib.STATUS_UNSUPPORTED
f = ctypes.c_void_p(0x1000)  # never dereferenced: every answer below is given on the host before any launch


def _tail(y=f, ld_y=None, lengths=f, off=f, gamma=f, beta=f, W=f, bias=f, out=f, out_lengths=f, B=2, T=7, Tpad=9, P=40, N=16, factor=3,
          eps=1e-3, dtype=1):
    """the default shape (P = 40) is outside the kernel's range: a call that passes every argument check answers UNSUPPORTED, no launch"""
    return _lib.load().tfasr_rnnt_block_tail_fwd(y, P if ld_y is None else ld_y, lengths, off, gamma, beta, W, bias, out, out_lengths, B, T, Tpad,
                                                 P, N, factor, eps, dtype, None)


def test_symbol_declared_exported_and_bound():
    lib = _lib.load()
    src = open(HEADER).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", src)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == NARGS
    assert lib.tfasr_abi_version() == _lib.ABI_VERSION
    assert re.search(r"#define\s+TFASR_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, src)
    assert {"lengths", "off", "factor", "Tpad", "out", "out_lengths", "eps"} <= set(inspect.signature(K.rnnt_block_tail_fwd).parameters)


def test_range_is_answered_unsupported():
    for dtype in (0, 1):
        assert _tail(dtype=dtype) == UNSUPPORTED                       # P % 32
        assert _tail(dtype=dtype, P=2048 + 32) == UNSUPPORTED          # P past 2048
        assert _tail(dtype=dtype, P=64, N=24) == UNSUPPORTED           # N % 16
        assert _tail(dtype=dtype, P=64, N=1024 + 16) == UNSUPPORTED    # N past 1024
        assert _tail(dtype=dtype, P=64, N=16, B=65536) == UNSUPPORTED  # one grid row per stream
    assert K.rnnt_block_tail_supported(1024, 320) and K.rnnt_block_tail_supported(2048, 1024) and K.rnnt_block_tail_supported(32, 16)
    assert not K.rnnt_block_tail_supported(40, 16) and not K.rnnt_block_tail_supported(64, 24)
    assert not K.rnnt_block_tail_supported(2080, 16) and not K.rnnt_block_tail_supported(64, 1040)


def test_wrong_arguments_are_answered_invalid():
    for kw in (dict(y=None), dict(gamma=None), dict(beta=None), dict(W=None), dict(out=None), dict(B=-1), dict(T=-1), dict(Tpad=6),
               dict(P=0), dict(N=0), dict(factor=0), dict(factor=2), dict(ld_y=39), dict(dtype=2), dict(dtype=-1), dict(eps=-1.0)):
        assert _tail(**kw) == INVALID, kw
    # optional arguments
    assert _tail(lengths=None, off=None, bias=None, out_lengths=None) == UNSUPPORTED
    # alignment is judged behind the range (the shape here is in range; the misaligned pointer ends the call before any launch)
    for kw in (dict(y=ctypes.c_void_p(0x1008)), dict(W=ctypes.c_void_p(0x1004)), dict(out=ctypes.c_void_p(0x1002)),
               dict(gamma=ctypes.c_void_p(0x1008)), dict(beta=ctypes.c_void_p(0x1008)), dict(bias=ctypes.c_void_p(0x1008)), dict(ld_y=36)):
        assert _tail(P=32, N=16, **kw) == INVALID, kw
