"""The causal dense Conv1D kernel (csrc/conv1d.hip) against the float64 oracle of tests/jasper_oracle.py, f32 and bf16: shapes across
the tile sizes and the utterance boundary, the fused epilogue, position independence bit for bit, and the streams' tail update.
Bars: the project's single-layer bars (tests/test_stream_gpu.py): f32 rtol 1e-4 / atol 1e-5, bf16 2e-2 / 2e-2 with the inputs and
weights rounded to bf16 before the oracle sees them."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

import jasper_oracle as JO

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
BAR = {torch.float32: dict(rtol=1e-4, atol=1e-5), torch.bfloat16: dict(rtol=2e-2, atol=2e-2)}


def _case(seed, B, T, Cin, Cout, Kk, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(Kk, Cin, Cout, generator=g) * (1.0 / np.sqrt(Kk * Cin))
    if dtype == torch.bfloat16:
        x, w = x.to(dtype).float(), w.to(dtype).float()
    return x, w, g


def _run(dev, dtype, x, w, **kw):
    wd = w.to(dev).contiguous()
    if dtype == torch.bfloat16:
        wd = K.conv1d_pack_weight(wd)
    kw = {k: (v.to(dev).to(dtype).contiguous() if k == "addend" and v is not None else (v.to(dev) if isinstance(v, torch.Tensor) else v))
          for k, v in kw.items()}
    y = K.conv1d_fwd(x.to(dev).to(dtype).contiguous(), wd, tuple(w.shape), **kw)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Cin,Cout", [(80, 256), (256, 384), (16, 16)])
@pytest.mark.parametrize("Kk,stride,dil", [(1, 1, 1), (11, 2, 1), (11, 1, 1), (25, 1, 1), (3, 1, 2), (32, 1, 1)])
def test_conv1d_against_the_oracle(dev, dtype, Cin, Cout, Kk, stride, dil):
    """B = 3: the first rows of batch rows 1 and 2 sit right behind another utterance's memory and must see zeros there.  T = 37 is no
    tile multiple, T = 1 the smallest, T = 130 more than one 128-row (bf16) and two 64-row (f32) tiles."""
    for T in (37, 1, 130):
        x, w, _ = _case(1000 * Kk + T + Cin, 3, T, Cin, Cout, Kk, dtype)
        y = _run(dev, dtype, x, w, stride=stride, dilation=dil)
        ref = JO.conv1d_causal(x, w, stride, dil)
        assert y.shape == ref.shape == (3, -(-T // stride), Cout)
        np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), **BAR[dtype], err_msg=f"T={T}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("with_addend", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_epilogue(dev, dtype, affine, with_addend, relu):
    B, T, Cin, Cout, Kk = 2, 37, 80, 96, 11
    x, w, g = _case(5, B, T, Cin, Cout, Kk, dtype)
    bias = torch.randn(Cout, generator=g) * 0.3
    scale = torch.rand(Cout, generator=g) + 0.5 if affine else None
    shift = torch.randn(Cout, generator=g) * 0.3 if affine else None
    addend = torch.randn(B, T, Cout, generator=g) if with_addend else None
    if addend is not None and dtype == torch.bfloat16:
        addend = addend.to(dtype).float()
    y = _run(dev, dtype, x, w, bias=bias, scale=scale, shift=shift, addend=addend, relu=relu)
    ref = JO.conv1d_causal(x, w) + bias.double()
    if affine:
        ref = ref * scale.double() + shift.double()
    if with_addend:
        ref = ref + addend.double()
    if relu:
        ref = torch.relu(ref)
        assert (y >= 0).all() and (y == 0).any()
    np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), **BAR[dtype])


def test_the_residual_branch_is_the_same_entry_point(dev):
    """sum_i BN_i(pw_i(res_i)) chained through `addend`, then the main convolution with that sum and the ReLU (JasperSubBlockResidual)"""
    g = torch.Generator().manual_seed(9)
    B, T = 2, 21
    r0, r1, x = torch.randn(B, T, 48, generator=g), torch.randn(B, T, 64, generator=g), torch.randn(B, T, 96, generator=g)
    p0, p1, w = torch.randn(1, 48, 96, generator=g) * 0.1, torch.randn(1, 64, 96, generator=g) * 0.1, torch.randn(13, 96, 96, generator=g) * 0.03
    s = [torch.rand(96, generator=g) + 0.5 for _ in range(3)]
    t = [torch.randn(96, generator=g) * 0.2 for _ in range(3)]
    a = _run(dev, torch.float32, r0, p0, scale=s[0], shift=t[0])
    a = _run(dev, torch.float32, r1, p1, scale=s[1], shift=t[1], addend=a.cpu())
    y = _run(dev, torch.float32, x, w, scale=s[2], shift=t[2], addend=a.cpu(), relu=True)
    ref = torch.relu(JO.conv1d_causal(x, w) * s[2].double() + t[2].double() + JO.conv1d_causal(r0, p0) * s[0].double() + t[0].double()
                     + JO.conv1d_causal(r1, p1) * s[1].double() + t[1].double())
    np.testing.assert_allclose(y.cpu().numpy(), ref.numpy(), **BAR[torch.float32])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Kk,stride,dil", [(11, 1, 1), (11, 2, 1), (3, 1, 2), (25, 1, 1)])
def test_position_independence_bit_for_bit(dev, dtype, Kk, stride, dil):
    """the same utterance alone, as row 2 of a batch of 3, behind real rows in a longer buffer, and through `lead`: torch.equal"""
    Cin, Cout, T = 80, 96, 150
    x, w, g = _case(77 + Kk, 1, T, Cin, Cout, Kk, dtype)
    bias = torch.randn(Cout, generator=g) * 0.2
    alone = _run(dev, dtype, x, w, bias=bias, stride=stride, dilation=dil, relu=True)
    other = torch.randn(2, T, Cin, generator=g)
    batch = _run(dev, dtype, torch.cat([other, x], 0), w, bias=bias, stride=stride, dilation=dil, relu=True)
    assert torch.equal(batch[2], alone[0])
    # second half of a longer T: an even offset (so the stride-2 phase agrees) that no tile size divides; its first (K - 1) * dil rows
    # are then real rows of the first half, so only the outputs whose taps all fall inside the copy can be compared
    off, pad = 70, (Kk - 1) * dil
    long = torch.cat([torch.randn(1, off, Cin, generator=g).to(dtype).float(), x], 1)
    moved = _run(dev, dtype, long, w, bias=bias, stride=stride, dilation=dil, relu=True)
    first = -(-pad // stride)  # output rows of `alone` from here on read no padding
    assert torch.equal(moved[0, off // stride + first:], alone[0, first:])
    # the streams' form: rows [s - pad, s) handed over as `lead` rows of real context give rows s / stride .. of the whole
    s0 = 64
    win = x[:, s0 - pad:]
    tail = _run(dev, dtype, win, w, bias=bias, stride=stride, dilation=dil, relu=True, lead=pad)
    assert torch.equal(tail[0], alone[0, s0 // stride:])
    # and a lead of zero rows is the causal padding itself
    zlead = _run(dev, dtype, torch.cat([torch.zeros(1, pad, Cin), x], 1), w, bias=bias, stride=stride, dilation=dil, relu=True, lead=pad)
    assert torch.equal(zlead, alone)


def test_unsupported_shapes_raise(dev):
    x = torch.zeros(1, 8, 24, device=dev)
    with pytest.raises(K._lib.TfasrUnsupported):
        K.conv1d_fwd(x, torch.zeros(3, 24, 16, device=dev), (3, 24, 16))
    x = torch.zeros(1, 8, 16, device=dev)
    with pytest.raises(K._lib.TfasrUnsupported):
        K.conv1d_fwd(x, torch.zeros(33, 16, 16, device=dev), (33, 16, 16))
    with pytest.raises(K._lib.TfasrUnsupported):
        K.conv1d_fwd(x, torch.zeros(3, 16, 16, device=dev), (3, 16, 16), stride=3)


@pytest.mark.parametrize("dtype", DT)
def test_tail_update(dev, dtype):
    g = torch.Generator().manual_seed(3)
    B, tail_rows, n, C = 4, 10, 8, 48
    tail = torch.randn(B, tail_rows, C, generator=g).to(dtype).to(dev)
    new = torch.randn(B, n, C, generator=g).to(dtype).to(dev)
    nvalid = [8, 0, 3, 1]
    win = torch.cat([tail, new], 1)
    before = tail.clone()
    K.conv1d_tail_update(win, torch.tensor(nvalid, dtype=torch.int32, device=dev), tail)
    torch.cuda.synchronize()
    for b, nv in enumerate(nvalid):
        assert torch.equal(tail[b], win[b, nv:nv + tail_rows]), b
    assert torch.equal(tail[1], before[1])  # an idle stream keeps its tail bit for bit
