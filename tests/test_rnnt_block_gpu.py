"""tfasr_rnnt_block_tail_fwd (csrc/rnnt_block.hip) against an f64 NumPy LayerNorm + Dense: masked rows computed from zeros whatever the
buffer holds, the zero rows of the next reduction, the reduced lengths, per-stream row offsets, a strided input, a variance-0 row, rows
past one workgroup's share, and the bits of a row not depending on the launch it sits in.

Tolerances are the ones tests/test_ops_gpu.py grants the last operation of the chain, the product with a bias, in the same type
(f32 rtol / atol 1e-4, bf16 3e-2; its LayerNorm bounds, 1e-5 / 2e-5 and 2e-2, are inside them); the reference sees the inputs and the
kernel rounded to the storage type, as there."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
EPS = 1e-3


def tol(dtype):
    return dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)


def make(B, T, P, N, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(B, T, P, generator=g) * 1.5 + 0.25).to(dtype)
    gamma, beta = torch.randn(P, generator=g) * 0.5 + 1.0, torch.randn(P, generator=g) * 0.5
    W = (torch.randn(P, N, generator=g) / np.sqrt(P)).to(dtype)
    bias = torch.randn(N, generator=g) * 0.5
    return y, gamma, beta, W, bias


def ref_rows(y, gamma, beta, W, bias):
    """f64: LN(rows) W + bias over the last axis of y [..., P]"""
    y = y.double().numpy()
    m = y.mean(-1, keepdims=True)
    v = ((y - m) ** 2).mean(-1, keepdims=True)
    ln = (y - m) / np.sqrt(v + EPS) * gamma.double().numpy() + beta.double().numpy()
    return ln @ W.double().numpy() + bias.double().numpy()


def reference(y, lens, gamma, beta, W, bias):
    """rows at and past lens[b] are computed from zeros"""
    ym = y.clone().float()
    for b, n in enumerate(lens):
        ym[b, n:] = 0.0
    return ref_rows(ym, gamma, beta, W, bias)


def device_weight(W, dtype, dev):
    if dtype == torch.float32:
        return W.to(dev).contiguous()
    return K.conv1d_pack_weight(W.float().to(dev).view(1, *W.shape).contiguous())


def run(dev, dtype, y, lens, gamma, beta, W, bias, factor=1, Tpad=None, off=None, out=None):
    N = W.shape[1]
    lens_dev = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    off_dev = None if off is None else torch.tensor(off, dtype=torch.int32, device=dev)
    out, olen = K.rnnt_block_tail_fwd(y, gamma.to(dev), beta.to(dev), device_weight(W, dtype, dev), bias.to(dev), N, lengths=lens_dev,
                                      off=off_dev, factor=factor, Tpad=Tpad, out=out, eps=EPS)
    torch.cuda.synchronize()
    return out.float().cpu().numpy(), olen.cpu().numpy()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("P,N", [(32, 16), (96, 48)])
def test_masked_rows_zero_rows_and_lengths(dev, dtype, P, N):
    """B = 3, T = 7, lengths (7, 4, 0), factor 3 with Tpad = 9; the masked rows of y hold NaN; one valid row is constant (variance 0)"""
    B, T, lens = 3, 7, [7, 4, 0]
    y, gamma, beta, W, bias = make(B, T, P, N, dtype, 100 + P)
    y[0, 2] = 1.5
    want = reference(y, lens, gamma, beta, W, bias)
    yd = y.clone()
    for b, n in enumerate(lens):
        yd[b, n:] = float("nan")
    out, olen = run(dev, dtype, yd.to(dev), lens, gamma, beta, W, bias, factor=3, Tpad=9)
    assert out.shape == (B, 9, N) and np.isfinite(out).all()
    np.testing.assert_allclose(out[:, :T], want, **tol(dtype))
    assert (out[:, T:] == 0).all()
    assert olen.tolist() == [3, 2, 0]
    # the constant row and every masked row are LN(0) W + bias = beta W + bias
    bw = ref_rows(torch.zeros(1, P), gamma, beta, W, bias)[0]
    for b, t in ((0, 2), (1, 4), (1, 6), (2, 0), (2, 6)):
        np.testing.assert_allclose(out[b, t], bw, **tol(dtype))
    # all masked rows are the same bits
    assert (out[1, 4:T] == out[2, 0]).all()


@pytest.mark.parametrize("dtype", DT)
def test_row_offsets_keep_the_rows_in_front(dev, dtype):
    """off = (2, 0, 1): the rows land behind each stream's carried rows, which are left alone; the rest of Tpad = 9 is zero"""
    B, T, P, N, lens, off = 3, 7, 96, 48, [7, 4, 0], [2, 0, 1]
    y, gamma, beta, W, bias = make(B, T, P, N, dtype, 7)
    want = reference(y, lens, gamma, beta, W, bias)
    buf = torch.full((B, 9, N), 7.0, dtype=dtype, device=dev)
    out, olen = run(dev, dtype, y.to(dev), lens, gamma, beta, W, bias, factor=3, Tpad=9, off=off, out=buf)
    for b in range(B):
        rows = min(T, 9 - off[b])
        assert (out[b, :off[b]] == 7.0).all()
        np.testing.assert_allclose(out[b, off[b]:off[b] + rows], want[b, :rows], **tol(dtype))
        assert (out[b, off[b] + rows:] == 0).all()
    assert olen.tolist() == [3, 2, 1]  # ceil((off + len) / 3)


@pytest.mark.parametrize("dtype", DT)
def test_strided_input_and_no_lengths(dev, dtype):
    B, T, P, N = 2, 5, 96, 48
    y, gamma, beta, W, bias = make(B, T, P, N, dtype, 11)
    wide = torch.full((B, T, 2 * P), float("nan"), dtype=dtype, device=dev)
    wide[:, :, :P] = y.to(dev)
    view = wide[:, :, :P]
    assert not view.is_contiguous()
    out, olen = run(dev, dtype, view, None, gamma, beta, W, bias)
    np.testing.assert_allclose(out, ref_rows(y.float(), gamma, beta, W, bias), **tol(dtype))
    assert olen.tolist() == [T, T]


@pytest.fixture(scope="module")
def long_case():
    """B = 2, T = 300: ten (bf16) / nineteen (f32) workgroups per stream; computed once per type"""
    cache = {}

    def get(dev, dtype):
        if dtype not in cache:
            B, T, P, N, lens = 2, 300, 96, 48, [300, 157]
            y, gamma, beta, W, bias = make(B, T, P, N, dtype, 3)
            out, olen = run(dev, dtype, y.to(dev), lens, gamma, beta, W, bias, factor=2, Tpad=300)
            cache[dtype] = (y, lens, gamma, beta, W, bias, out, olen)
        return cache[dtype]

    return get


@pytest.mark.parametrize("dtype", DT)
def test_rows_past_one_workgroup(dev, dtype, long_case):
    y, lens, gamma, beta, W, bias, out, olen = long_case(dev, dtype)
    np.testing.assert_allclose(out, reference(y, lens, gamma, beta, W, bias), **tol(dtype))
    assert olen.tolist() == [150, 79]


@pytest.mark.parametrize("dtype", DT)
def test_a_row_has_the_same_bits_in_any_launch(dev, dtype, long_case):
    """rows 100 .. 104 of stream 1 again, as a one-stream launch of five rows behind an offset of three: another B, T, Tpad, off, tile and
    place in the tile - bit-equal"""
    y, lens, gamma, beta, W, bias, out, _ = long_case(dev, dtype)
    part = y[1:2, 100:105].contiguous()
    buf = torch.zeros(1, 8, W.shape[1], dtype=dtype, device=dev)
    small, olen = run(dev, dtype, part.to(dev), [5], gamma, beta, W, bias, factor=4, Tpad=8, off=[3], out=buf)
    assert (small[0, 3:8] == out[1, 100:105]).all()
    assert olen.tolist() == [2]
    # ... and a masked row is the same bits wherever it is computed
    masked, _ = run(dev, dtype, part.to(dev), [0], gamma, beta, W, bias)
    assert (masked[0] == out[1, 200]).all()


def test_outside_the_range_raises_and_launches_nothing(dev):
    y = torch.zeros(1, 2, 40, device=dev)
    with pytest.raises(_lib.TfasrUnsupported):
        K.rnnt_block_tail_fwd(y, torch.ones(40, device=dev), torch.zeros(40, device=dev), torch.zeros(40, 16, device=dev), None, 16)
