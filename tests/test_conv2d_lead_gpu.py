"""conv2d_fwd(lead = kh - 1) (kernels.py over tfasr_conv2d_fwd, csrc/conv2d_gen.hip): a causal Conv2D over [carried tail | new rows] gives,
bit for bit, the matching output rows of the offline causal call over the whole sequence - with the tail the last kh - 1 rows in front of
the piece, zeros at the sequence's start.  The kernel itself is held to the float64 oracle by tests/test_conv2d_gen_gpu.py; this is the
chain from a streamed conv block to it."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

pytestmark = pytest.mark.gpu
LAYERS = [((5, 7, 1, 16), (2, 2), 16, 23), ((3, 5, 16, 16), (1, 2), 16, 11),  # the tiny DeepSpeech2's two conv blocks
          ((11, 41, 1, 32), (2, 2), 160, 24)]                                # uni.yml.j2's first block


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape,strides,F,T", LAYERS)
def test_pieces_over_a_carried_tail_equal_the_offline_rows(dev, dtype, shape, strides, F, T):
    kh, kw, Cin, Cout = shape
    st = strides[0]
    g = torch.Generator().manual_seed(T + F + kh)
    B = 2
    x = torch.randn(B, T, F, Cin, generator=g).to(dtype).to(dev)
    w = (torch.randn(kh, kw, Cin, Cout, generator=g) * (1.0 / np.sqrt(kh * kw * Cin))).to(dev)
    wd = K.conv2d_pack_weight(w) if dtype == torch.bfloat16 else w
    bias, scale, shift = (torch.randn(Cout, generator=g) * 0.1).to(dev), (torch.rand(Cout, generator=g) + 0.5).to(dev), (torch.randn(Cout, generator=g) * 0.2).to(dev)
    kw_ = dict(bias=bias, scale=scale, shift=shift, relu=True, strides=strides, padding="causal")
    ref = K.conv2d_fwd(x, wd, shape, **kw_)
    assert ref.shape[1] == -(-T // st) and float(ref.float().abs().max()) > 0.1
    # pieces: multiples of the time stride in the middle of the sequence, whatever is left (odd where T is) at its end
    for piece in (st, 2 * st, 4 * st, T):
        tail = torch.zeros(B, kh - 1, F * Cin, dtype=dtype, device=dev)
        t0 = 0
        while t0 < T:
            n = min(piece, T - t0)
            win = torch.cat([tail, x[:, t0:t0 + n].reshape(B, n, F * Cin)], 1)
            y = K.conv2d_fwd(win.view(B, kh - 1 + n, F, Cin), wd, shape, lead=kh - 1, **kw_)
            assert y.shape == (B, -(-n // st), ref.shape[2], Cout)
            assert torch.equal(_bits(y), _bits(ref[:, t0 // st:t0 // st + y.shape[1]])), (piece, t0)
            K.conv1d_tail_update(win, torch.full((B,), n, dtype=torch.int32, device=dev), tail)
            assert torch.equal(_bits(tail), _bits(win[:, n:])), (piece, t0)
            t0 += n


def test_lead_zero_is_the_plain_call_and_other_leads_are_refused(dev):
    x = torch.randn(1, 6, 16, 1, device=dev)
    w = torch.randn(5, 7, 1, 16, device=dev)
    a = K.conv2d_fwd(x, w, (5, 7, 1, 16), strides=(2, 2), padding="causal")
    b = K.conv2d_fwd(x, w, (5, 7, 1, 16), strides=(2, 2), padding="causal", lead=0)
    assert torch.equal(_bits(a), _bits(b))
    for kw in (dict(padding="causal", lead=3), dict(padding="same", lead=4), dict(padding="causal", lead=-1)):
        with pytest.raises(ValueError, match="lead"):
            K.conv2d_fwd(x, w, (5, 7, 1, 16), strides=(2, 2), **kw)
    with pytest.raises(ValueError, match="lead"):
        K.conv2d_fwd(x[:, :3], w, (5, 7, 1, 16), strides=(2, 2), padding="causal", lead=4)
