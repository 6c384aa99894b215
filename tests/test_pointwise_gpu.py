"""The kernels of csrc/elementwise.hip, each against a plain torch-CPU float64 statement of the same operation, at the sizes and on the
dispatch branches the whole-model tests never reach: the packed and dense transducer joint, cast_colsum_many, colsum and the shared
attention biases on their vector and scalar kernels, and every grid-stride loop past its first pass.

References are computed from inputs already rounded to the storage type, so only the kernel's own arithmetic is judged.  Tolerances:
  * pure data movement (cast, gather, masks): bitwise;
  * f32 element-wise results: the values the suite already holds these kernels to (test_ops_gpu.py: joint rtol 1e-5 / atol 1e-6, Adam
    rtol 1e-5, GLU 1e-5 / 1e-5 forward and 1e-4 / 1e-5 backward);
  * an f32 sum of n terms: |y - ref| <= n * 2^-23 * S + 1e-7 with S the float64 sum of the absolute terms.  A sum of n terms in any
    order is off by at most (n - 1) * 2^-24 * S; the factor two leaves room for the two roundings inside a term (a product, a scale).
    A value the sum starts from counts as one more term;
  * a bf16 result of an f32 computation: one bf16 ulp, 2^-7 * |ref|, on top of the f32 bound.
At a million terms the sum bound is far wider than one lost or doubled element, so the large sums also run on small-integer data, where
every partial sum is an integer (or a multiple of the power-of-two scale) below 2^24: f32 addition is then exact in any order and the
result has to be the reference bitwise."""
import functools

import numpy as np
import pytest
import torch

from oracle import conformer_ref as R
from tensorflowasr_amd import kernels as K

pytestmark = pytest.mark.gpu

# Mirrored from csrc/elementwise.hip.  flat_grid() launches at most 4096 blocks of 256 threads, so a scalar kernel takes a second
# grid-stride iteration past GRID_THREADS elements and a kernel that moves VEC elements per lane (ld8 / st8) past GRID_THREADS * VEC.
GRID_THREADS = 4096 * 256
VEC = 8

F32, BF16 = torch.float32, torch.bfloat16
DT = [F32, BF16]
DT_IDS = ["f32", "bf16"]
F64 = torch.float64
BF16_ULP = 2.0 ** -7
F32_SUM = 2.0 ** -23


def rt(x, dtype):
    """round-trip through the storage dtype so the reference sees the same inputs"""
    return x.to(dtype).float()


@functools.lru_cache(maxsize=None)
def _randn(n, seed):
    """shared, read-only standard normal f32 vector (one draw per (n, seed) for the whole module)"""
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _within(y, ref, bound, what):
    """|y - ref| <= bound element-wise (ref / bound float64 on the host).  A NaN in y fails."""
    y = y.detach().double().cpu().reshape(ref.shape)
    bound = torch.broadcast_to(torch.as_tensor(bound, dtype=F64), ref.shape)
    ok = (y - ref).abs() <= bound
    if not bool(ok.all()):
        i = tuple((~ok).nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} values outside the bound; first at {i}: "
                             f"got {float(y[i])!r}, want {float(ref[i])!r}, bound {float(bound[i]):.3e}")


def _elem_bound(ref, dtype, rtol=1e-5, atol=1e-6):
    a = rtol * ref.abs() + atol
    return a if dtype == F32 else BF16_ULP * ref.abs() + a


def _sum_bound(ref, S, n, dtype=F32):
    a = torch.as_tensor(n, dtype=F64) * F32_SUM * S + 1e-7
    return a if dtype == F32 else BF16_ULP * ref.abs() + a


def _poison(dev, dtype, *shapes):
    """Fill blocks of the sizes a wrapper is about to torch.empty with NaN and release them: the caching allocator hands the same blocks
    back, so an element the kernel skips reads NaN rather than the result a previous case left there.  (Best effort; no assertion
    relies on it.)"""
    bufs = [torch.full(s, float("nan"), dtype=dtype, device=dev) for s in shapes]
    torch.cuda.synchronize()
    del bufs


# ------------------------------------------------------------------------------------------------------------------ packed joint
# name -> (T, U1, logit lengths, label lengths).  "ragged": a one-frame utterance, an empty transcript, an utterance with no cell.
# "gap": the cell-less utterance in the middle, T = 11.  "wide": U1 = 11, the longest utterance last.  (T = 11 / U1 = 11: the four
# threadIdx.y streams of joint_bwd_packed_kernel get counts that are no multiple of four.)
LATTICES = {
    "ragged": (9, 7, [9, 4, 1, 0], [6, 2, 0, 0]),
    "full": (9, 7, [9, 9, 9, 9], [6, 6, 6, 6]),
    "gap": (11, 7, [11, 0, 5, 10], [6, 3, 1, 0]),
    "wide": (6, 11, [3, 2, 1, 6], [5, 9, 0, 10]),
}


def _lattice(name):
    T, U1, tl, ul = LATTICES[name]
    off = np.zeros(len(tl) + 1, np.int64)  # as conformer.py builds it
    off[1:] = np.cumsum([t * (u + 1) for t, u in zip(tl, ul)])
    return T, U1, tl, ul, off, int(off[-1])


def _lattice_dev(name, dev):
    T, U1, tl, ul, off, total = _lattice(name)
    return (torch.from_numpy(off).to(dev), torch.tensor(ul, dtype=torch.int32, device=dev), torch.tensor(tl, dtype=torch.int32, device=dev))


@functools.lru_cache(maxsize=None)
def _joint_inputs(name, J, dtype):
    T, U1, tl, ul, off, total = _lattice(name)
    B = len(tl)
    g = torch.Generator().manual_seed(1000 + J)
    enc, pred = rt(torch.randn(B, T, J, generator=g), dtype), rt(torch.randn(B, U1, J, generator=g), dtype)
    dh = rt(torch.randn(total, J, generator=g), dtype)
    rows = [torch.tanh(enc[b, :tl[b], None].double() + pred[b, None, :ul[b] + 1].double()).reshape(-1, J) for b in range(B)]
    return enc, pred, dh, torch.cat(rows)  # h: float64 [total, J], row by row


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("J", [8, 512, 640, 2056])
def test_joint_packed_forward(dev, dtype, J):
    """tfasr_joint_fwd_packed.  J = 8: more u-lanes than U + 1; 512: J / 8 divides the 256 threads; 640: it does not (16 idle threads);
    2056: J / 8 = 257, the flat kernel with its binary search over cell_off.  On the full lattice the packed result is the dense
    kernel's, bitwise."""
    for name in ("ragged", "gap", "full"):
        T, U1, tl, ul, off, total = _lattice(name)
        enc, pred, _, href = _joint_inputs(name, J, dtype)
        off_dev, ul_dev, _ = _lattice_dev(name, dev)
        e, p = enc.to(dev).to(dtype), pred.to(dev).to(dtype)
        _poison(dev, dtype, (total, J))
        h = K.joint_fwd_packed(e, p, off_dev, ul_dev, total)
        assert h.shape[0] == total and h.shape == (total, J)
        _within(h, href, _elem_bound(href, dtype), f"packed joint forward, {name}")
        if name == "full":
            assert torch.equal(h, K.joint_fwd(e, p).view(-1, J))


@pytest.mark.parametrize("with_h", [False, True], ids=["h-none", "h-given"])
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("J", [8, 640, 1032])
@pytest.mark.parametrize("name", list(LATTICES))
def test_joint_packed_backward(dev, name, dtype, J, with_h):
    """tfasr_joint_bwd_packed: the two segment sums, with h == NULL (dh already carries the tanh' factor: what the model passes) and with
    h.  J = 1032: a second blockIdx.y whose only live lanes are columns 1024..1031.  The outputs are the wrapper's torch.empty buffers:
    every padded row (t >= logit_len or u > label_len) has to come back exactly zero.  (With h a term is dh * (1 - h^2): the factor is one
    fused multiply-add, rounded once, so it loses nothing where h is close to 1; a separate square and subtraction, as torch-CPU f32 does
    them, can miss the sum bound there.)"""
    T, U1, tl, ul, off, total = _lattice(name)
    B = len(tl)
    _, _, dh, href = _joint_inputs(name, J, dtype)
    hq = rt(href.float(), dtype)  # the stored activations
    terms = dh.double() * (1.0 - hq.double() ** 2) if with_h else dh.double()
    denc_ref, dpred_ref = torch.zeros(B, T, J, dtype=F64), torch.zeros(B, U1, J, dtype=F64)
    denc_S, dpred_S = torch.zeros(B, T, J, dtype=F64), torch.zeros(B, U1, J, dtype=F64)
    denc_pad, dpred_pad = torch.ones(B, T, dtype=torch.bool), torch.ones(B, U1, dtype=torch.bool)
    denc_n, dpred_n = torch.zeros(B, T, 1, dtype=F64), torch.zeros(B, U1, 1, dtype=F64)
    for b in range(B):
        g = terms[off[b]:off[b + 1]].view(tl[b], ul[b] + 1, J)
        denc_ref[b, :tl[b]], denc_S[b, :tl[b]] = g.sum(1), g.abs().sum(1)
        dpred_ref[b, :ul[b] + 1], dpred_S[b, :ul[b] + 1] = g.sum(0), g.abs().sum(0)
        denc_n[b, :tl[b]], dpred_n[b, :ul[b] + 1] = ul[b] + 1, tl[b]
        denc_pad[b, :tl[b]] = False
        if tl[b] > 0:
            dpred_pad[b, :ul[b] + 1] = False
    off_dev, ul_dev, tl_dev = _lattice_dev(name, dev)
    _poison(dev, dtype, (B, T, J), (B, U1, J))
    denc, dpred = K.joint_bwd_packed(hq.to(dev).to(dtype) if with_h else None, dh.to(dev).to(dtype), off_dev, ul_dev, tl_dev, B, T, U1)
    assert denc.shape == (B, T, J) and dpred.shape == (B, U1, J)
    _within(denc, denc_ref, _sum_bound(denc_ref, denc_S, denc_n, dtype), f"packed joint backward, denc, {name}")
    _within(dpred, dpred_ref, _sum_bound(dpred_ref, dpred_S, dpred_n, dtype), f"packed joint backward, dpred, {name}")
    assert bool((denc.cpu()[denc_pad] == 0).all()), f"{name}: padded encoder rows are not zero"
    # (an utterance without frames has no cell at all: its u <= label_len rows are sums of nothing and count as padding)
    assert bool((dpred.cpu()[dpred_pad] == 0).all()), f"{name}: padded prediction rows are not zero"


# ------------------------------------------------------------------------------------------------------------------- dense joint
def _dense_ref(enc, pred):
    return torch.tanh(enc[:, :, None].double() + pred[:, None].double())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("B,T,U1,J", [(1, 3, 2, 1032), (2, 5, 1, 8), (1, 1, 9, 640)])
def test_joint_dense(dev, dtype, B, T, U1, J):
    """tfasr_joint_fwd / tfasr_joint_bwd.  J = 1032: joint_bwd_kernel's second blockIdx.y; U1 = 1 and T = 1: sums of one term."""
    g = torch.Generator().manual_seed(J + T)
    enc, pred = rt(torch.randn(B, T, J, generator=g), dtype), rt(torch.randn(B, U1, J, generator=g), dtype)
    dh = rt(torch.randn(B, T, U1, J, generator=g), dtype)
    href = _dense_ref(enc, pred)
    h = K.joint_fwd(enc.to(dev).to(dtype), pred.to(dev).to(dtype))
    _within(h, href, _elem_bound(href, dtype), "dense joint forward")
    hq = rt(href.float(), dtype)
    terms = dh.double() * (1.0 - hq.double() ** 2)
    _poison(dev, dtype, (B, T, J), (B, U1, J))
    denc, dpred = K.joint_bwd(hq.to(dev).to(dtype), dh.to(dev).to(dtype))
    _within(denc, terms.sum(2), _sum_bound(terms.sum(2), terms.abs().sum(2), U1, dtype), "dense joint backward, denc")
    _within(dpred, terms.sum(1), _sum_bound(terms.sum(1), terms.abs().sum(1), T, dtype), "dense joint backward, dpred")


def test_joint_dense_past_one_grid(dev):
    """joint_fwd_kernel moves VEC elements per lane: B * T * U1 * J = GRID_THREADS * VEC + 97792, so its grid-stride loop repeats."""
    B, T, U1, J = 2, 130, 51, 640
    assert B * T * U1 * J == GRID_THREADS * VEC + 97792
    enc = rt(_randn(B * T * J, 11).view(B, T, J), BF16)
    pred = rt(_randn(B * U1 * J, 12).view(B, U1, J), BF16)
    href = _dense_ref(enc, pred)
    _poison(dev, BF16, (B, T, U1, J))
    h = K.joint_fwd(enc.to(dev).to(BF16), pred.to(dev).to(BF16))
    _within(h, href, _elem_bound(href, BF16), "dense joint forward past one grid")


def test_joint_tanh_saturating_and_tiny_arguments(dev):
    """tanh_fast = 1 - 2 / (exp2(c x) + 1) where that form overflows (exp2 -> inf), underflows (-> 0) or cancels (x -> 0): finite, within
    2e-7 of tanh (the error stated beside tanh_fast in common.h, doubled) and exactly +-1 once the exponential has left the f32 range.
    The sums are exact: one operand carries the value, the other is zero."""
    mags = [0.0, 1e-8, 1e-3, 20.0, 44.0, 89.0, 1e4]
    s = torch.tensor([sg * m for m in mags for sg in (1.0, -1.0)], dtype=F32)  # includes -0.0
    n, J = s.numel(), 8
    enc, pred = torch.zeros(1, n, J), torch.zeros(1, 1, J)
    enc[0, :, :] = s[:, None]
    h = K.joint_fwd(enc.to(dev), pred.to(dev)).cpu().view(n, J)
    h2 = K.joint_fwd(torch.zeros(1, 1, J, device=dev), s.view(1, n, 1).expand(1, n, J).contiguous().to(dev)).cpu().view(n, J)
    want = torch.tanh(s.double())[:, None].expand(n, J)
    for got in (h, h2):
        assert bool(torch.isfinite(got).all())
        _within(got, want, 2e-7, "tanh_fast")
        sat = s.abs() >= 89.0
        assert torch.equal(got[sat], torch.sign(s[sat])[:, None].expand(-1, J))


# ------------------------------------------------------------------------------------------------------------- cast_colsum_many
@pytest.mark.parametrize("nmat,rows,C", [(3, 17, 64), (2, 130, 68), (65, 3, 4), (4, 64, 256)])
def test_cast_colsum_many(dev, nmat, rows, C):
    """tfasr_cast_colsum_many: bf16 copies of f32 matrices spaced `stride` apart and their column sums ADDED to per-matrix buffers, NULL
    entries skipped.  (17, 64): fewer rows than one 64-row pass; (130, 68): three passes, a second column block with four live columns;
    (65, 3, 4): the wrapper's second launch (64 matrices per launch); (4, 64, 256): exactly one full pass, four full column blocks.
    The gap between matrices is never read (1e30 there) nor written (sentinel in y)."""
    g = torch.Generator().manual_seed(nmat * 1000 + rows)
    stride = rows * C + 12
    x = torch.full((nmat, stride), 1e30)
    x[:, :rows * C] = torch.randn(nmat, rows * C, generator=g)
    init = torch.randn(nmat, C, generator=g)
    skip = [b % 3 == 1 for b in range(nmat)]
    xd = x.to(dev)
    y = torch.full((nmat, stride), -7.0, dtype=BF16, device=dev)
    sums = init.to(dev)  # one table: a row whose entry is None must keep its values
    K.cast_colsum_many(xd, y, stride, nmat, rows, C, [None if skip[b] else sums[b] for b in range(nmat)])
    yc = y.cpu()
    assert torch.equal(yc[:, :rows * C], x[:, :rows * C].to(BF16))
    assert bool((yc[:, rows * C:] == -7.0).all())
    xm = x[:, :rows * C].view(nmat, rows, C).double()
    ref, S = init.double() + xm.sum(1), init.double().abs() + xm.abs().sum(1)
    live = torch.tensor([not k for k in skip])
    _within(sums[live.to(dev)], ref[live], _sum_bound(ref[live], S[live], rows + 1), "cast_colsum_many sums")
    assert torch.equal(sums.cpu()[~live], init[~live])


def test_cast_colsum_many_rejects_a_width_off_the_vector(dev):
    rows, C, stride = 4, 6, 24
    x = torch.zeros(2, stride, device=dev)
    y = torch.zeros(2, stride, dtype=BF16, device=dev)
    with pytest.raises(K._lib.TfasrUnsupported):
        K.cast_colsum_many(x, y, stride, 2, rows, C, [torch.zeros(C, device=dev), None])


# ---------------------------------------------------------------------------------------------------- colsum, bias2 on every branch
def _strided(vals, ld, dtype, dev):
    """[rows, ld] device buffer holding vals in its first C columns and 1e30 in the padding"""
    buf = torch.full((vals.shape[0], ld), 1e30, dtype=dtype, device=dev)
    buf[:, :vals.shape[1]] = vals.to(dev).to(dtype)
    return buf


# (dtype, rows, C, row stride, small-integer data).  The kernels choose the 16-byte bf16 kernel iff C % 8 == 0 and stride % 8 == 0.
BRANCHES = {
    # three column blocks of 256, the last with 8 live columns; more rows than one pass of the capped grid holds, ragged last pass
    "vec": (BF16, 7000, 520, 520, True),
    "vec-small": (BF16, 33, 8, 8, False),
    "vec-padded": (BF16, 300, 264, 272, False),
    # C % 8 != 0: the scalar kernels on bf16; rows * C = GRID_THREADS + 176, so bias2_fwd_kernel's grid-stride loop repeats
    "scalar-width": (BF16, GRID_THREADS // 36 + 5, 36, 36, True),
    "scalar-stride": (BF16, 333, 40, 44, False),
    "f32": (F32, 777, 100, 100, False),
    "f32-padded": (F32, 130, 100, 108, False),
}


@pytest.mark.parametrize("case", list(BRANCHES))
def test_colsum_and_bias2_branches(dev, case):
    """tfasr_colsum, tfasr_bias2_fwd, tfasr_bias2_bwd on the vector and the scalar kernels, with padded row strides (the padding is neither
    read into a sum nor written) and sums that ADD to non-zero outputs.  The small-integer cases must be exact (module docstring)."""
    dtype, rows, C, ld, ints = BRANCHES[case]
    g = torch.Generator().manual_seed(rows + C)
    if ints:
        d1, d2 = _ints((rows, C), -4, 4, rows), _ints((rows, C), -4, 4, rows + 1)
        u, v, init1, init2 = (_ints((C,), -9, 9, C + k) for k in range(4))
        scale = 0.5
    else:
        d1, d2 = rt(torch.randn(rows, C, generator=g), dtype), rt(torch.randn(rows, C, generator=g), dtype)
        u, v, init1, init2 = (torch.randn(C, generator=g) for _ in range(4))
        scale = 0.75
    # colsum
    xbuf = _strided(d1, ld, dtype, dev)
    out = init1.to(dev)
    K.colsum(xbuf[:, :C], out, scale=scale)
    ref = init1.double() + scale * d1.double().sum(0)
    S = init1.double().abs() + scale * d1.double().abs().sum(0)
    _within(out, ref, _sum_bound(ref, S, rows + 1), "colsum")
    if ints:
        assert torch.equal(out.cpu().double(), ref)
    # bias2 forward
    y1, y2 = K.bias2_fwd(xbuf[:, :C], ld, u.to(dev), v.to(dev), rows, C)
    r1, r2 = d1.double() + u.double(), d1.double() + v.double()
    _within(y1, r1, _elem_bound(r1, dtype), "bias2_fwd y1")
    _within(y2, r2, _elem_bound(r2, dtype), "bias2_fwd y2")
    # bias2 backward
    dx = torch.full((rows, ld), 1e30, dtype=dtype, device=dev)
    du, dv = init1.to(dev), init2.to(dev)
    K.bias2_bwd(d1.to(dev).to(dtype), d2.to(dev).to(dtype), dx, ld, du, dv, rows, C)
    rdx = d1.double() + d2.double()
    _within(dx[:, :C], rdx, _elem_bound(rdx, dtype), "bias2_bwd dx")
    assert torch.equal(dx[:, C:], torch.full((rows, ld - C), 1e30, dtype=dtype, device=dev))
    for got, init, d, what in ((du, init1, d1, "du"), (dv, init2, d2, "dv")):
        ref = init.double() + d.double().sum(0)
        _within(got, ref, _sum_bound(ref, init.double().abs() + d.double().abs().sum(0), rows + 1), f"bias2_bwd {what}")
        if ints:
            assert torch.equal(got.cpu().double(), ref)


def test_bias2_forward_vector_kernel_past_one_grid(dev):
    """bias2_fwd_vec_kernel handles VEC columns per lane: rows * C = GRID_THREADS * VEC + 1592."""
    C = 520
    rows = GRID_THREADS * VEC // C + 4
    assert rows * C == GRID_THREADS * VEC + 1592
    x = rt(_randn(rows * C, 21).view(rows, C), BF16)
    u, v = _randn(C, 22), _randn(C, 23)
    _poison(dev, BF16, (rows, C), (rows, C))
    y1, y2 = K.bias2_fwd(x.to(dev).to(BF16), C, u.to(dev), v.to(dev), rows, C)
    r1, r2 = x.double() + u.double(), x.double() + v.double()
    _within(y1, r1, _elem_bound(r1, BF16), "bias2_fwd y1")
    _within(y2, r2, _elem_bound(r2, BF16), "bias2_fwd y2")


# ------------------------------------------------------------------------------------------------- past one grid: scalar kernels
N_SCALAR = GRID_THREADS + 257


def _f32(v):
    """a host scalar as the f32 the C ABI receives"""
    return float(np.float32(v))


@pytest.mark.parametrize("shadow", [False, True], ids=["plain", "shadow"])
@pytest.mark.parametrize("n_reg", [0, 1000, N_SCALAR])
def test_adam_past_one_grid(dev, n_reg, shadow):
    """adam_kernel over GRID_THREADS + 257 parameters with the L2 term on none, on the first 1000 and on all of them (the full-vector
    comparison covers both sides of the n_reg boundary).  The shadow is the cast of the updated parameters, bitwise."""
    n = N_SCALAR
    p, gr = _randn(n, 31), _randn(n, 32)
    gg = torch.Generator().manual_seed(33)
    m, v = torch.rand(n, generator=gg) * 0.1, torch.rand(n, generator=gg) * 0.01
    step, lr, b1, b2, eps, wd, l2, gs = 7, _f32(3e-3), _f32(0.9), _f32(0.98), _f32(1e-9), _f32(1e-2), _f32(1e-2), 0.5
    geff = gr.double() * gs
    geff[:n_reg] += 2 * l2 * p[:n_reg].double()
    pr, mr, vr = R.adam_step(p.double(), geff, m.double(), v.double(), step, lr, b1, b2, eps, wd)
    pd, md, vd = p.to(dev), m.to(dev), v.to(dev)
    sh = torch.full((n,), 99.0, dtype=BF16, device=dev) if shadow else None
    K.adam(pd, gr.to(dev), md, vd, n_reg, lr, step, b1, b2, eps, wd, l2, gs, shadow=sh)
    _within(pd, pr, 1e-5 * pr.abs() + 1e-6, "adam p")
    _within(md, mr, 1e-5 * mr.abs() + 1e-7, "adam m")
    _within(vd, vr, 1e-5 * vr.abs() + 1e-8, "adam v")
    if shadow:
        assert torch.equal(sh, K.cast(pd, torch.empty(n, dtype=BF16, device=dev)))
        assert torch.equal(sh.cpu(), pd.cpu().to(BF16))


@pytest.mark.parametrize("alpha", [1.0, -0.25])
@pytest.mark.parametrize("n", [1, 255, N_SCALAR])
def test_axpy(dev, n, alpha):
    x, y = _randn(n, 41), _randn(n, 42)
    buf = torch.full((n + 8,), 5.0, device=dev)  # the kernel must stop at n
    buf[:n] = y.to(dev)
    K.axpy(buf[:n], x.to(dev), alpha)
    ref = y.double() + alpha * x.double()
    _within(buf[:n], ref, 1e-5 * ref.abs() + 1e-6, "axpy")
    assert bool((buf[n:] == 5.0).all())


@pytest.mark.parametrize("n_sum", [N_SCALAR, GRID_THREADS + 1, 1000])
def test_sumsq(dev, n_sum):
    """sumsq_kernel adds the sum of the first n_sum squares to a non-zero out[0]: normal data within the sum bound, then values in
    -3..3 whose sum of squares (< 9 * 2^20 < 2^24) is exact in any order."""
    n = N_SCALAR
    p = _randn(n, 51)
    out = torch.full((1,), 3.0, device=dev)
    K.sumsq(p.to(dev), n_sum, out)
    sq = p[:n_sum].double() ** 2
    ref, S = 3.0 + sq.sum()[None], 3.0 + sq.sum()[None]
    _within(out, ref, _sum_bound(ref, S, n_sum + 1), "sumsq")
    q = _ints((n,), -3, 3, 52)
    out = torch.full((1,), 5.0, device=dev)
    K.sumsq(q.to(dev), n_sum, out)
    assert float(out) == 5.0 + float((q[:n_sum].double() ** 2).sum())


@pytest.mark.parametrize("mask_value", [0.0, -3.5])
@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_specaugment_past_one_grid(dev, dtype, mask_value):
    """specaug_kernel over B * T * F = GRID_THREADS + 9584 elements, bitwise against the oracle's mask application on the rounded input:
    masks that end exactly on the last bin / frame, zero-width masks, masks in the part of the tensor the second grid pass covers, no
    frequency masks (fmask = None) and no time masks."""
    B, F = 3, 80
    T = GRID_THREADS // (B * F) + 40
    assert B * T * F == GRID_THREADS + 9584
    feat = rt(_randn(B * T * F, 61).view(B, T, F), dtype)
    fm = np.array([[(F - 5 - b, 5 + b), (10, 0), (20 + b, 7)] for b in range(B)], np.int32)
    tm = np.array([[(T - 7, 7), (100, 0), (T // 2 + b, 50), (T - 30, 4)] for b in range(B)], np.int32)
    for fmask, tmask in ((fm, tm), (None, tm), (fm, None)):
        ref = R.specaugment_apply(feat.numpy(), fmask, tmask, mask_value)
        x = feat.to(dev).to(dtype)
        K.specaugment(x, None if fmask is None else torch.from_numpy(fmask).to(dev), None if tmask is None else torch.from_numpy(tmask).to(dev),
                      mask_value)
        np.testing.assert_array_equal(x.float().cpu().numpy(), ref)
        assert (ref == mask_value).any() and (ref[B - 1, T - 20:] != mask_value).any()


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
@pytest.mark.parametrize("V", [3, 5000])
def test_embedding_past_one_grid(dev, dtype, V):
    """embedding_fwd / embedding_bwd with rows * E = GRID_THREADS + 104.  V = 3: every atomic of the scatter collides.  The gather is
    bitwise; the scatter adds to a non-zero table, within the sum bound on normal data and exact on small integers."""
    E = 40
    rows = GRID_THREADS // E + 3
    assert rows * E == GRID_THREADS + 104
    g = torch.Generator().manual_seed(V)
    idx = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    table = torch.randn(V, E, generator=g)
    _poison(dev, dtype, (rows, E))
    out = K.embedding_fwd(idx.to(dev), table.to(dev), dtype)
    assert torch.equal(out.cpu(), table[idx.long()].to(dtype))
    count = torch.bincount(idx.long(), minlength=V).double()[:, None]
    for ints in (False, True):
        dout = _ints((rows, E), -8, 8, V + 1) if ints else rt(_randn(rows * E, 71).view(rows, E), dtype)
        init = _ints((V, E), -9, 9, V + 2) if ints else table
        dt_ = init.to(dev)
        K.embedding_bwd(idx.to(dev), dout.to(dev).to(dtype), dt_)
        ref = init.double().index_add(0, idx.long(), dout.double())
        S = init.double().abs().index_add(0, idx.long(), dout.double().abs())
        _within(dt_, ref, _sum_bound(ref, S, count + 1), "embedding_bwd")
        if ints:
            assert torch.equal(dt_.cpu().double(), ref)


# --------------------------------------------------------------------------------------- past one grid: 8-wide kernels with tails
N_VEC = GRID_THREADS * VEC + 13


@pytest.mark.parametrize("n", [1, 7, 8, 1003, N_VEC])
@pytest.mark.parametrize("src_dtype,dst_dtype", [(F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)],
                         ids=["f32-bf16", "bf16-f32", "f32-f32", "bf16-bf16"])
def test_cast(dev, src_dtype, dst_dtype, n):
    """cast_kernel: n / 8 chunks of VEC elements, then a scalar tail of n % 8; n = 1 and 7 are all tail, 8 has none, N_VEC repeats the
    chunk loop and has a 5-element tail.  Bitwise, and nothing is written past n."""
    src = _randn(n, 81).to(src_dtype)
    buf = torch.full((n + 8,), -7.0, dtype=dst_dtype, device=dev)
    K.cast(src.to(dev), buf[:n])
    got = buf.cpu()
    assert torch.equal(got[:n], src.to(dst_dtype))
    assert bool((got[n:] == -7.0).all())


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_glu_past_one_grid(dev, dtype):
    """glu_fwd_kernel / glu_bwd_kernel with rows * C = GRID_THREADS * VEC + 256 outputs, C = 264 (no power of two: the row / column split
    of a chunk index is a real division)."""
    C = 264
    rows = GRID_THREADS * VEC // C + 1
    assert rows * C == GRID_THREADS * VEC + 256
    x = rt(_randn(rows * 2 * C, 91).view(rows, 2 * C), dtype)
    dy = rt(_randn(rows * C, 92).view(rows, C), dtype)
    a, b = x[:, :C].double(), x[:, C:].double()
    s = torch.sigmoid(b)
    xd = x.to(dev).to(dtype)
    _poison(dev, dtype, (rows, C))
    y = K.glu_fwd(xd)
    ref = a * s
    _within(y, ref, _elem_bound(ref, dtype, 1e-5, 1e-5), "glu_fwd")
    del y, ref
    _poison(dev, dtype, (rows, 2 * C))
    dx = K.glu_bwd(xd, dy.to(dev).to(dtype))
    ref = torch.cat([dy.double() * s, dy.double() * a * s * (1.0 - s)], 1)
    _within(dx, ref, _elem_bound(ref, dtype, 1e-4, 1e-5), "glu_bwd")


@pytest.mark.parametrize("dtype", DT, ids=DT_IDS)
def test_dropout_value_depends_on_seed_and_index_only(dev, dtype):
    """dropout_kernel has no host model; what the code promises is that element i is a function of (seed, i) alone.  So a short run (one
    pass, 3-element scalar tail) equals the head of a run whose chunk loop repeats (and whose tail is elsewhere), bitwise."""
    n1, n2, p, seed = 100_003, N_VEC, 0.1, 4711
    buf = torch.full((n2 + 8,), -7.0, dtype=dtype, device=dev)
    K.dropout(torch.ones(n2, dtype=dtype, device=dev), p, seed, out=buf[:n2])
    y1 = K.dropout(torch.ones(n1, dtype=dtype, device=dev), p, seed)
    assert torch.equal(y1, buf[:n1])
    assert bool((buf[n2:] == -7.0).all())
    y2 = buf[:n2]
    keep = (y2 != 0).float().mean().item()
    assert abs(keep - 0.9) < 0.005  # (the bound of test_model_gpu.py)
    kept = y2[y2 != 0].double()
    assert float((kept - 1.0 / 0.9).abs().max()) <= (1e-6 if dtype == F32 else BF16_ULP) / 0.9


def test_gauss_noise_value_depends_on_seed_and_index_only(dev):
    n1, n2, seed = 100_003, N_SCALAR, 123
    buf = torch.zeros(n2 + 8, device=dev)
    K.gauss_noise(buf[:n2], 0.5, seed)
    y1 = K.gauss_noise(torch.zeros(n1, device=dev), 0.5, seed)
    assert torch.equal(y1, buf[:n1])
    assert bool((buf[n2:] == 0).all())
    a = buf[:n2].cpu().numpy()
    assert abs(a.mean()) < 3e-3 and abs(a.std() - 0.5) < 3e-3  # (the bounds of test_dropin_api_gpu.py)
