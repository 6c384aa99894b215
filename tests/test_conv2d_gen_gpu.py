"""The general Conv2D kernel (csrc/conv2d_gen.hip) against the float64 oracle of tests/ds2_oracle.py, f32 and bf16: the two shipped
DeepSpeech2 layers under both padding rules, a kernel wider than half the frequency axis (padding wider than the data on both sides),
every channel tile, the fused epilogue, and position independence bit for bit.
Bars: the project's single-layer bars (tests/test_jasper_conv1d_gpu.py): f32 rtol 1e-4 / atol 1e-5, bf16 2e-2 / 2e-2 with the inputs and
weights rounded to bf16 before the oracle sees them."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

import ds2_oracle as DO

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
BAR = {torch.float32: dict(rtol=1e-4, atol=1e-5), torch.bfloat16: dict(rtol=2e-2, atol=2e-2)}


def _case(seed, B, T, F, shape, dtype):
    kh, kw, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, F, Cin, generator=g)
    w = torch.randn(kh, kw, Cin, Cout, generator=g) * (1.0 / np.sqrt(kh * kw * Cin))
    if dtype == torch.bfloat16:
        x, w = x.to(dtype).float(), w.to(dtype).float()
    return x, w, g


def _run(dev, dtype, x, w, **kw):
    wd = w.to(dev).contiguous()
    if dtype == torch.bfloat16:
        wd = K.conv2d_pack_weight(wd)
    kw = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in kw.items()}
    y = K.conv2d_fwd(x.to(dev).to(dtype).contiguous(), wd, tuple(w.shape), **kw)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("padding", ["same", "causal"])
@pytest.mark.parametrize("shape,strides,F,T", [((11, 41, 1, 32), (2, 2), 160, 23), ((11, 21, 32, 32), (1, 2), 80, 12)])
def test_the_shipped_layers(dev, dtype, padding, shape, strides, F, T):
    """base.yml.j2 / uni.yml.j2 conv blocks 0 and 1 at B = 2"""
    x, w, _ = _case(T + F, 2, T, F, shape, dtype)
    y = _run(dev, dtype, x, w, strides=strides, padding=padding)
    ref = DO.conv2d(x, w, strides, padding)
    assert y.shape == ref.shape == (2, -(-T // strides[0]), -(-F // strides[1]), shape[3])
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), **BAR[dtype])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("padding", ["same", "causal"])
@pytest.mark.parametrize("Cout", [48, 16, 96, 128])
def test_wide_kernel_short_axes_and_channel_tiles(dev, dtype, padding, Cout):
    """(5, 7, 16 -> Cout) strides (3, 2) on F = 16: kw > F / 2, so the zero padding is wider than the data on both sides; T = 1, 2 and 37
    (no tile multiple, more than one tile of output rows); B = 3: rows 1 and 2 sit right behind another sample's memory and must read
    zeros there.  Cout 16 / 48 / 96 / 128: half a channel tile, one and a half, three, four."""
    for T in (1, 2, 37):
        x, w, _ = _case(100 * Cout + T, 3, T, 16, (5, 7, 16, Cout), dtype)
        y = _run(dev, dtype, x, w, strides=(3, 2), padding=padding)
        ref = DO.conv2d(x, w, (3, 2), padding)
        assert y.shape == ref.shape == (3, -(-T // 3), 8, Cout)
        np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), **BAR[dtype], err_msg=f"T={T}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape,strides,F", [((3, 5, 1, 16), (1, 1), 19), ((16, 48, 16, 32), (2, 1), 40), ((1, 1, 32, 16), (1, 2), 7),
                                             ((4, 6, 48, 32), (1, 2), 33)])
def test_other_shapes(dev, dtype, shape, strides, F):
    """frequency stride 1 with one input channel (odd element offsets in the bf16 kernel's window reads), the largest kernel, a 1 x 1
    kernel, even kernel sizes ("same" pads one more behind than in front) with Cin = 48 (a k-step spans two frequency positions unevenly)"""
    for padding in ("same", "causal"):
        x, w, _ = _case(F, 2, 9, F, shape, dtype)
        y = _run(dev, dtype, x, w, strides=strides, padding=padding)
        ref = DO.conv2d(x, w, strides, padding)
        np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), **BAR[dtype], err_msg=padding)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_epilogue(dev, dtype, affine, with_bias, relu):
    x, w, g = _case(5, 2, 7, 16, (5, 7, 16, 48), dtype)
    bias = torch.randn(48, generator=g) * 0.3 if with_bias else None
    scale = torch.rand(48, generator=g) + 0.5 if affine else None
    shift = torch.randn(48, generator=g) * 0.3 if affine else None
    y = _run(dev, dtype, x, w, bias=bias, scale=scale, shift=shift, relu=relu, strides=(2, 2), padding="same")
    ref = DO.affine(DO.conv2d(x, w, (2, 2), "same"), bias, scale, shift, relu)
    if relu:
        assert (y >= 0).all() and (y == 0).any()
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), **BAR[dtype])


@pytest.mark.parametrize("dtype", DT)
def test_position_independence_bit_for_bit(dev, dtype):
    """a sample alone against the same sample as row 2 of 3; T = 37 against its first 20 rows under causal padding (an output row reads
    input rows at or before 3 t' only, so output rows 0 .. 6 of the short run see the same data: other tiles, same bits)"""
    x, w, _ = _case(77, 3, 37, 16, (5, 7, 16, 48), dtype)
    for padding in ("same", "causal"):
        y3 = _run(dev, dtype, x, w, strides=(3, 2), padding=padding)
        y1 = _run(dev, dtype, x[2:3], w, strides=(3, 2), padding=padding)
        assert torch.equal(y3[2:3], y1), padding
    ys = _run(dev, dtype, x[:, :20].contiguous(), w, strides=(3, 2), padding="causal")
    assert ys.shape[1] == 7 and torch.equal(ys, y3[:, :7])
    # stride 1: every output row of the short run
    y = _run(dev, dtype, x, w, strides=(1, 2), padding="causal")
    ys = _run(dev, dtype, x[:, :20].contiguous(), w, strides=(1, 2), padding="causal")
    assert torch.equal(ys, y[:, :20])


def test_channel_affine(dev):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 7, 48, generator=g)
    scale, shift = torch.rand(48, generator=g) + 0.5, torch.randn(48, generator=g) * 0.3
    for dtype in DT:
        xd = x.to(dtype)
        y = K.channel_affine_fwd(xd.to(dev), scale.to(dev), shift.to(dev), relu=True)
        ref = DO.affine(xd.double(), None, scale, shift, True)
        np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), **BAR[dtype])
