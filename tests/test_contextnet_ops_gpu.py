"""Every ABI entry of csrc/contextnet.hip through its kernels.py wrapper against a float64 torch-CPU restatement of the same operation
(the formulas of oracle/contextnet_ref.py: se_module, the residual add + swish of encoder_forward, the causal stride as "every s-th
row"), in f32 and bf16, at the channel counts, lengths and sizes where these kernels change behaviour:

  * C in {8, 40, 256, 640, 1280}: one lane, a partial 256-channel slab, one slab, 2.5 slabs, 5 slabs of se_reduce_kernel;
  * odd T with stride 2 and 3 (T2 = ceil(T / s); the backward zeroes every row that was not sampled);
  * lengths mixing T, 1, a mid value and one above T (clamped to T), and lengths = None (never 0: the reference does not define it);
  * one shape per elementwise kernel above 16.8 M elements (flat_grid caps the grid at 8192 workgroups of 256 lanes x 8 elements),
    so the grid-stride loop goes round more than once.

Inputs are rounded to bf16 and then cast, so both storage types and the f64 reference see the same numbers.

Tolerances (derived, not tuned):
  * f32 outputs: rtol 1e-5 against the f64 result;
  * sums over T rows: additionally atol = T * 2^-23 * max|term|;
  * results formed as a sum of terms that can cancel (se_bwd_apply: dy*s + dpool/len; the activation derivatives: 1 + z(1 - s) has a
    root at z = -1.28, 1 - s underflows its relative precision for large z): every term is rounded relative to the TERM, not to the
    result, so additionally atol = 4 * 2^-23 * |term| element by element (the same reasoning as the reduction rule, for 2-3 terms);
  * bf16 outputs: one rounding of the f32 value: rtol 2^-8, atol 2^-8 * max|ref|;
  * exact (assert_equal): subsample forward (a copy), subsample backward (a copy plus zeros), se_scale in f32 (a single multiply),
    ACT_NONE with b = None (a copy).
"""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.kernels import ACT_NONE, ACT_SIGMOID, ACT_SWISH

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
EPS32, EPS16 = 2.0 ** -23, 2.0 ** -8
CHANNELS = [8, 40, 256, 640, 1280]
BIG = (32, 1100, 512)  # 18.0 M elements > 8192 * 256 * 8 = 16.8 M: the grid-stride loops wrap
WRAP = 8192 * 256 * 8


def _rand(shape, seed, scale=1.0):
    """bf16-representable values as f32 (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).float()


def _close(got, ref, dtype, atol_terms=None, what=""):
    """got: GPU tensor; ref: f64 CPU.  atol_terms: f64 tensor broadcastable to ref, the per-element magnitude whose f32 rounding the
    result carries (already multiplied by its count)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    if dtype == torch.bfloat16:
        tol = EPS16 * ref.abs() + EPS16 * float(ref.abs().max())
    else:
        tol = 1e-5 * ref.abs()
    if atol_terms is not None:
        tol = tol + EPS32 * atol_terms
    bad = (got - ref).abs() > tol
    assert not bool(bad.any()), (what, int(bad.sum()), float(((got - ref).abs() - tol).max()))


def _lengths(B, T):
    """T, 1, a mid value, one above T (the kernels clamp), then a spread."""
    base = [T, 1, max(1, T // 2), T + 5, max(1, T - 1), min(T, 3)]
    return [base[i % len(base)] for i in range(B)]


# ------------------------------------------------------------------------------------------------ row subsampling (exact)
SUB_SHAPES = [(3, 57, 8, 2), (2, 101, 40, 3), (2, 33, 256, 2), (2, 7, 640, 3), (2, 9, 1280, 2), (2, 1, 8, 2), (1, 2, 40, 3), (2, 64, 256, 2),
              (3, 10, 8, 1)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,C,s", SUB_SHAPES)
def test_rows_subsample_forward_is_every_sth_row_and_backward_scatters_with_zeros(dev, dtype, B, T, C, s):
    T2 = -(-T // s)
    x = _rand((B, T, C), 1).to(dtype)
    y = K.rows_subsample_fwd(x.to(dev), s)
    assert y.shape == (B, T2, C)
    assert torch.equal(y.cpu(), x[:, ::s])
    dy = _rand((B, T2, C), 2).to(dtype)
    dx = K.rows_subsample_bwd(dy.to(dev), T, s)
    ref = torch.zeros(B, T, C, dtype=dtype)
    ref[:, ::s] = dy
    assert dx.shape == (B, T, C)
    assert torch.equal(dx.cpu(), ref)
    assert int((dx.cpu() != 0).any(-1).sum()) <= B * T2  # every row that was not sampled is zero


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_rows_subsample_above_one_grid_sweep(dev, dtype):
    """Output of the forward and output of the backward both above 16.8 M elements, odd lengths."""
    B, C = 32, 512
    T = 2201                                     # forward: T2 = 1101, 18.0 M output elements
    x = _rand((B, T, C), 3).to(dtype)
    y = K.rows_subsample_fwd(x.to(dev), 2)
    assert y.numel() > WRAP and torch.equal(y.cpu(), x[:, ::2])
    T = 1101                                     # backward: 18.0 M output elements, T2 = 551
    dy = x[:, :551].contiguous()
    dx = K.rows_subsample_bwd(dy.to(dev), T, 2)
    ref = torch.zeros(B, T, C, dtype=dtype)
    ref[:, ::2] = dy
    assert dx.numel() > WRAP and torch.equal(dx.cpu(), ref)
    dx3 = K.rows_subsample_bwd(x[:, :367].contiguous().to(dev), T, 3)
    ref.zero_()
    ref[:, ::3] = x[:, :367]
    assert torch.equal(dx3.cpu(), ref)


# ------------------------------------------------------------------------------------------------ squeeze-and-excite
SE_SHAPES = [(4, 57, 8), (4, 33, 40), (6, 100, 256), (5, 47, 640), (4, 176, 1280), (3, 1, 40), (3, 7, 640), (2, 9, 1280)]


def _mask(lens, T):
    ln = torch.tensor(lens).clamp(max=T)
    return (torch.arange(T)[None, :] < ln[:, None]).double()[..., None], ln.double()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("use_len", [True, False], ids=["ragged", "nolen"])
@pytest.mark.parametrize("B,T,C", SE_SHAPES)
def test_se_pool_is_the_masked_mean(dev, dtype, use_len, B, T, C):
    x = _rand((B, T, C), 4)
    lens = _lengths(B, T) if use_len else [T] * B
    mask, ln = _mask(lens, T)
    ref = (x.double() * mask).sum(1) / ln[:, None]
    terms = (x.double().abs() * mask).amax((1, 2))[:, None] / ln[:, None]      # max |x / len| per utterance
    len_dev = torch.tensor(lens, dtype=torch.int32).to(dev) if use_len else None
    got = K.se_pool(x.to(dtype).to(dev), len_dev)
    assert got.dtype == torch.float32
    _close(got, ref, torch.float32, T * terms, "se_pool")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("B,T,C", SE_SHAPES)
def test_se_scale_forward_and_its_scale_gradient(dev, dtype, B, T, C):
    x, dy, s = _rand((B, T, C), 5), _rand((B, T, C), 6), torch.sigmoid(_rand((B, C), 7)).to(torch.bfloat16).float()
    y = K.se_scale_fwd(x.to(dtype).to(dev), s.to(dev))
    if dtype == torch.float32:
        assert torch.equal(y.cpu(), x * s[:, None, :])                           # one IEEE multiply
    else:
        _close(y, x.double() * s.double()[:, None, :], dtype, None, "se_scale_fwd")
    ds = K.se_scale_bwd_reduce(x.to(dtype).to(dev), dy.to(dtype).to(dev))
    assert ds.dtype == torch.float32
    prod = x.double() * dy.double()
    _close(ds, prod.sum(1), torch.float32, T * prod.abs().amax(1), "se_scale_bwd_reduce")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("use_len", [True, False], ids=["ragged", "nolen"])
@pytest.mark.parametrize("B,T,C", SE_SHAPES)
def test_se_bwd_apply_adds_the_pool_gradient_to_the_valid_frames(dev, dtype, use_len, B, T, C):
    dy, s, dpool = _rand((B, T, C), 8), torch.sigmoid(_rand((B, C), 9)).to(torch.bfloat16).float(), _rand((B, C), 10, 4.0)
    lens = _lengths(B, T) if use_len else [T] * B
    mask, ln = _mask(lens, T)
    t1 = dy.double() * s.double()[:, None, :]
    t2 = mask * (dpool.double() / ln[:, None])[:, None, :]
    len_dev = torch.tensor(lens, dtype=torch.int32).to(dev) if use_len else None
    got = K.se_bwd_apply(dy.to(dtype).to(dev), s.to(dev), dpool.to(dev), len_dev)
    _close(got, t1 + t2, dtype, 4 * (t1.abs() + t2.abs()), "se_bwd_apply")
    pad = (mask == 0).expand_as(t1)
    if dtype == torch.float32 and bool(pad.any()):                               # padded frames: exactly dy * s
        assert torch.equal(got.cpu()[pad], (dy * s[:, None, :])[pad])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_se_kernels_above_one_grid_sweep(dev, dtype):
    B, T, C = BIG
    assert B * T * C > WRAP
    x, s, dpool = _rand((B, T, C), 11), torch.sigmoid(_rand((B, C), 12)).to(torch.bfloat16).float(), _rand((B, C), 13, 4.0)
    lens = [T - 37 * b for b in range(B)]
    lens[3], lens[7] = 1, T + 9
    mask, ln = _mask(lens, T)
    xd, len_dev = x.to(dtype).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev)
    y = K.se_scale_fwd(xd, s.to(dev))
    if dtype == torch.float32:
        assert torch.equal(y.cpu(), x * s[:, None, :])
    else:
        _close(y, x.double() * s.double()[:, None, :], dtype, None, "se_scale_fwd big")
    t1 = x.double() * s.double()[:, None, :]
    t2 = mask * (dpool.double() / ln[:, None])[:, None, :]
    got = K.se_bwd_apply(xd, s.to(dev), dpool.to(dev), len_dev)
    _close(got, t1 + t2, dtype, 4 * (t1.abs() + t2.abs()), "se_bwd_apply big")
    del t1, t2, got, y
    ref = (x.double() * mask).sum(1) / ln[:, None]
    terms = (x.double().abs() * mask).amax((1, 2))[:, None] / ln[:, None]
    _close(K.se_pool(xd, len_dev), ref, torch.float32, T * terms, "se_pool big")
    dy = x.flip(0)
    prod = x.double() * dy.double()
    _close(K.se_scale_bwd_reduce(xd, dy.to(dtype).to(dev)), prod.sum(1), torch.float32, T * prod.abs().amax(1), "se_scale_bwd_reduce big")


# ------------------------------------------------------------------------------------------------ residual add + activation
def _act64(z, act):
    sg = torch.sigmoid(z)
    if act == ACT_SWISH:
        return z * sg, sg * (1 + z * (1 - sg))
    if act == ACT_SIGMOID:
        return sg, sg * (1 - sg)
    return z, torch.ones_like(z)


def _check_add_act(dev, dtype, shape, act, with_b, seed):
    a, b, dy = _rand(shape, seed, 3.0), (_rand(shape, seed + 1, 3.0) if with_b else None), _rand(shape, seed + 2)
    ad, bd, dyd = a.to(dtype).to(dev), (b.to(dtype).to(dev) if with_b else None), dy.to(dtype).to(dev)
    z = a.double() + (b.double() if with_b else 0.0)         # bf16 + bf16 is exact in f32 (8-bit mantissas, exponents within 16)
    y64, d64 = _act64(z, act)
    y, d = K.add_act_fwd(ad, bd, act), K.add_act_bwd(ad, bd, dyd, act)
    if act == ACT_NONE and not with_b:
        assert torch.equal(y.cpu(), a.to(dtype)) and torch.equal(d.cpu(), dy.to(dtype))
        return
    if act == ACT_NONE and dtype == torch.float32:
        assert torch.equal(y.cpu(), a + b) and torch.equal(d.cpu(), dy)
        return
    _close(y, y64, dtype, None, "add_act_fwd")
    _close(d, dy.double() * d64, dtype, 4 * dy.double().abs(), "add_act_bwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("with_b", [True, False], ids=["a+b", "a"])
@pytest.mark.parametrize("act", [ACT_NONE, ACT_SWISH, ACT_SIGMOID], ids=["none", "swish", "sigmoid"])
@pytest.mark.parametrize("shape", [(3, 57, 8), (2, 33, 40), (5, 1280), (2, 101, 640)])
def test_add_act_forward_and_backward(dev, dtype, with_b, act, shape):
    _check_add_act(dev, dtype, shape, act, with_b, 20)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("act,with_b", [(ACT_SWISH, True), (ACT_NONE, True), (ACT_SIGMOID, False), (ACT_NONE, False)],
                         ids=["swish-a+b", "none-a+b", "sigmoid-a", "none-a"])
def test_add_act_above_one_grid_sweep(dev, dtype, act, with_b):
    assert int(np.prod(BIG)) > WRAP
    _check_add_act(dev, dtype, BIG, act, with_b, 30)
