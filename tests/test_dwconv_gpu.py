"""Every depthwise-convolution / GLU entry point and launch branch of csrc/dwconv.hip and csrc/elementwise.hip against the float64
restatements of tests/dwconv_oracle.py (conventions of tests/test_norm_gpu.py, whose `hold` and `exact` are used here).

Entry point                        kernel instantiations                                              test
tfasr_dwconv_fwd                   dwconv_tile_kernel<false,false,8>, <false> (KB = 32);              test_conv_pair_kernel_sizes, _time_seams, _channel_slabs
                                   dwconv_fwd_kernel<float|bf16_t>                                    test_conv_scalar_kernels
tfasr_dwconv_bwd_data              dwconv_tile_kernel<true,false,8>, <true>;                          (the same tests: every case runs both directions)
                                   dwconv_bwd_data_kernel<float|bf16_t>                               test_conv_scalar_kernels
tfasr_dwconv_bwd_weight_ws,        dwconv_wgrad_tile_kernel<3|5|7|15|31|32> with `part`,              test_weight_gradient_tile_route
  ..._workspace_size               dwconv_wgrad_reduce_kernel (empty, single and 4-unrolled slices)
tfasr_dwconv_bwd_weight_ws,        dwconv_bwd_weight_kernel<float|bf16_t>                             test_weight_gradient_fallback
  tfasr_dwconv_bwd_weight          (K without a tile instantiation, workspace short / NULL, f32, C % 8, off 16 bytes)
tfasr_dwconv_bwd_weight_many       dwconv_wgrad_tile_many_kernel<3|5|7|15|31|32>,                     test_weight_gradient_of_many_products,
                                   dwconv_wgrad_reduce_many_kernel; one by one otherwise              ..._many_falls_back_one_by_one, test_status_codes
tfasr_dwconv_fwd_stats             dwconv_tile_kernel<false,false,8,true>, <false,false,32,true>      test_forward_with_statistics
tfasr_glu_dwconv_fwd_stats         dwconv_tile_kernel<false,false,32,true,true> (GIN)                 test_gated_forward_with_statistics
tfasr_dwconv_bwd_data_glu          dwconv_tile_kernel<true,true> (GLU)                                test_data_gradient_with_glu_backward
tfasr_bn_dwconv_bwd_data_glu       dwconv_tile_kernel<true,true,32,false,false,true> (BNIN)           test_batchnorm_backward_data_gradient_glu_backward
tfasr_glu_fwd, tfasr_glu_bwd       glu_fwd_kernel<float|bf16_t>, glu_bwd_kernel<float|bf16_t>         test_glu
INVALID_VALUE / UNSUPPORTED                                                                           test_status_codes
dwconv_wgrad_tile_kernel<K> with part == nullptr (f32 atomics): UNREACHABLE, tfasr_dwconv_pair_try keeps `wgrad_tile = false`; not enabled.
tfasr_stream_glu_dwconv_fwd and tfasr_block_dwconv_wgrad_all (forwards to the `many` route) are outside this file.
Not tested: weight / bias pointers off 8 bytes.  The tile kernel loads the taps of a channel pair 8 bytes at a time and nothing checks their
alignment; every caller passes whole float32 tensors.

Inputs are rounded to the storage type first and the reference is computed from the rounded values.  Every activation lives inside a larger
buffer, with guards (a multiple of 8 elements, so the 16-byte checks of the launchers still pass) in front and behind: input guards hold
NaN, so a read outside the tensor that reaches a result fails; outputs and their guards are pre-filled with NaN, an element the kernel does
not write fails its comparison, and the guards must be bit-unchanged afterwards.  The partial-sum workspace is NaN before every call.
Backward and fused kernels get fin / bstats / g / dcv that the TEST chose, never the output of the GPU forward.

Exact cases (indexing): x, dy, a in {-1, -.5, 0, .5, 1}, w in {-1, 0, 1} at density 1/2, b = 0 (sigmoid = 1/2: a sigmoid(0) sits on a bf16
grid point that a 1-ulp v_rcp_f32 cannot move), non-zero lattice values in every destination that is added to: every float32 sum is exact in
any order, and dw, dbias, the statistics (each copy, and their sum), dgamma / dbeta and the bf16 y / dx / g / dglu must equal the reference
bit for bit.
Random cases (numerics), Gaussian mean 0.3, std 1.5, the constants of test_norm_gpu.py:
    elementwise outputs      |gpu - ref| <= 2^-20 M   (+ 2^-8 |ref| for a bf16 output), M = sum of |term| of the element
    sums over rows           |gpu - ref| <= 2^-18 sum |term|  per column
Chained quantities (y from g in GIN, dglu from dcv in BNIN, the statistics from y) take their reference from the intermediate the GPU
stored, read back; that intermediate is held to the oracle in the same test.  Every comparison prints max |gpu - ref| / bound first."""
import ctypes
import math

import pytest
import torch

import dwconv_oracle as DO
import norm_oracle as NO
from tensorflowasr_amd import kernels as K
from test_norm_gpu import BF, F32, K_BF16, K_ELEM, K_SUM, NAN, exact, gauss, gen, hold, lattice, pick

pytestmark = pytest.mark.gpu

# Tile constants, from the launch arithmetic of csrc/dwconv.hip and csrc/elementwise.hip
TGD = 16       # forward / data gradient: output steps per thread group; a workgroup owns 2 TGD = 32 steps (and K - 1 halo rows)
TG = 32        # weight gradient: steps per thread group; a workgroup owns 2 TG = 64 steps
SLAB = 256     # channels per workgroup of the tile kernels (128 lanes x 2 channels), staged in 16-byte pieces of 8
DW_TT = 8      # scalar forward / data-gradient kernels: steps per block
DW_WT = 64     # scalar weight-gradient kernel: steps per block
SLICES = 16    # dwconv_wgrad_reduce*_kernel: slices the partial slabs of a channel slab are reduced in
GLU_PASS = 256 * 16 * 256  # flat_grid(): <= 256 * 16 blocks x 256 threads, one 8-element piece each per trip

INVALID, UNSUPPORTED = 1, 3
HALF = (-1.0, -0.5, 0.0, 0.5, 1.0)
TAPS = (-1.0, 0.0, 0.0, 1.0)

RATIOS = []  # (what, max |got - ref| / bound) of every held() since it was last cleared (tests/test_dwconv_oracle.py reports them)


def _id(v):
    if isinstance(v, torch.dtype):
        return {BF: "bf16", F32: "f32"}[v]
    return "-".join(str(_id(e) or e) for e in v) if isinstance(v, tuple) else None


# ------------------------------------------------------------------------------------------------------------------------ helpers
def held(what, got, ref, M, k=K_ELEM, bf16=False):
    bound = k * M + (K_BF16 * ref.abs() if bf16 else 0.0)
    err = (got.detach().double().cpu().reshape(ref.shape) - ref).abs()
    RATIOS.append((what, float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())))
    hold(what, got, ref, M, k=k, bf16=bf16)


def bits_equal(what, got, ref):
    """got == ref bit for bit; ref (float64) must be a value of got's type"""
    if got.dtype == BF:
        assert torch.equal(ref.bfloat16().double(), ref), f"{what}: the reference itself is not a bf16 value"
    exact(what, got, ref)


def same(kind, what, got, ref, M, k=K_ELEM):
    if kind == "exact":
        bits_equal(what, got, ref)
    else:
        held(what, got, ref, M, k=k, bf16=got.dtype == BF)


def guard_len(width):
    return (40 * width + 7) // 8 * 8  # 40 rows: more than the K - 1 <= 31 rows a window could reach outside


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def put(t, dev, off=0):
    """`t` on the device between NaN guards; `off` elements past the 16-byte boundary"""
    g, n = guard_len(t.shape[-1]), t.numel()
    buf = torch.full((2 * g + n + 8,), NAN, dtype=t.dtype, device=dev)
    v = buf[g + off:g + off + n].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


class Out:
    """an output tensor of NaN between NaN guards"""

    def __init__(self, dev, shape, dtype, off=0):
        g, n = guard_len(shape[-1]), math.prod(shape)
        self.buf = torch.full((2 * g + n + 8,), NAN, dtype=dtype, device=dev)
        self.lo, self.hi = g + off, g + off + n
        self.v = self.buf[self.lo:self.hi].view(shape)
        self.snap = _bits(self.buf).clone()

    def done(self, what):
        """the guards are bit-unchanged; returns the tensor on the CPU"""
        b = _bits(self.buf)
        assert torch.equal(b[:self.lo], self.snap[:self.lo]) and torch.equal(b[self.hi:], self.snap[self.hi:]), f"{what}: written outside the tensor"
        return self.v.detach().cpu().clone()

    def untouched(self):
        return torch.equal(_bits(self.buf), self.snap)


def dev_(t, dev):
    return None if t is None else t.to(dev, copy=True)


def nan_ws(dev, nbytes):
    return torch.full((max(nbytes // 4, 1),), NAN, dtype=F32, device=dev)


def ws_size(B, T, C, Kk):
    n = ctypes.c_size_t(0)
    K.check(K._L().tfasr_dwconv_bwd_weight_workspace_size(B, T, C, Kk, ctypes.byref(n)), "dwconv_bwd_weight_workspace_size")
    assert n.value == B * ((T + 2 * TG - 1) // (2 * TG)) * ((C + SLAB - 1) // SLAB) * (Kk + 1) * SLAB * 4
    return n.value


def acts(g, kind, shape, dtype):
    return pick(g, shape, HALF).to(dtype) if kind == "exact" else gauss(g, shape, dtype)


def grads(g, kind, shape, dtype):
    return pick(g, shape, HALF).to(dtype) if kind == "exact" else torch.randn(*shape, generator=g).to(dtype)


def taps(g, kind, Kk, C, bias):
    if kind == "exact":
        return pick(g, (Kk, C), TAPS), pick(g, (C,), HALF) if bias else None
    return torch.randn(Kk, C, generator=g) * 0.5, torch.randn(C, generator=g) if bias else None


def gated(g, kind, shape, dtype):
    """the GLU's input a | b; exact: b = 0"""
    x = acts(g, kind, shape[:-1] + (2 * shape[-1],), dtype)
    if kind == "exact":
        x[..., shape[-1]:] = 0
    return x


# ------------------------------------------------------------------------------------------- forward and data gradient (plain)
def make_conv(case, kind):
    dtype, B, T, C, Kk, bias, off = case
    g = gen(11, B, T, C, Kk, bias, off, kind == "exact")
    w, b = taps(g, kind, Kk, C, bias)
    return dict(x=acts(g, kind, (B, T, C), dtype), dy=grads(g, kind, (B, T, C), dtype), w=w, bias=b)


def run_conv(dev, case, inp):
    dtype, B, T, C, Kk, bias, off = case
    x, dy, w, b = put(inp["x"], dev, off), put(inp["dy"], dev, off), dev_(inp["w"], dev), dev_(inp["bias"], dev)
    y, dx = Out(dev, (B, T, C), dtype, off), Out(dev, (B, T, C), dtype, off)
    K.check(K._L().tfasr_dwconv_fwd(K._p(x), K._p(w), K._p(b), K._p(y.v), B, T, C, Kk, K._dt(x), K._stream()), "dwconv_fwd")
    K.check(K._L().tfasr_dwconv_bwd_data(K._p(dy), K._p(w), K._p(dx.v), B, T, C, Kk, K._dt(x), K._stream()), "dwconv_bwd_data")
    return dict(y=y.done("y"), dx=dx.done("dx"))


def check_conv(case, kind, inp, out):
    f, b = DO.dwconv_fwd(inp["x"], inp["w"], inp["bias"]), DO.dwconv_bwd_data(inp["dy"], inp["w"])
    same(kind, "y", out["y"], f["y"], f["M_y"])
    same(kind, "dx", out["dx"], b["dx"], b["M_dx"])


# (dtype, B, T, C, K, bias, elements off 16 bytes)
CONV_SIZES = [(BF, 2, 33, 144, Kk, bias, 0) for Kk in (1, 3, 5, 8, 9, 15, 31, 32) for bias in (False, True)]  # KB = 8 | KB = 32
CONV_SEAMS = ([(BF, 3, T, 8, Kk, True, 0) for T in (1, 15, 16, 17, 31, 32, 33, 65, 97) for Kk in (5, 31)]
              + [(BF, 2, 29, 8, 31, False, 0), (BF, 2, 30, 8, 31, False, 0), (BF, 2, 30, 8, 32, False, 0), (BF, 2, 31, 8, 32, False, 0)])  # T = K-2, K-1
CONV_SLABS = [(BF, 2, 33, C, Kk, C != 264, 0) for C in (8, 144, 256, 264, 520) for Kk in (5, 15)]
CONV_SCALAR = [(F32, 2, 9, 40, 5, True, 0), (F32, 3, 65, 77, 31, False, 0), (F32, 2, 64, 300, 32, True, 0), (F32, 2, 7, 77, 1, True, 0),
               (BF, 2, 65, 100, 31, True, 0), (BF, 3, 9, 77, 5, False, 0), (BF, 2, 63, 77, 32, True, 0), (BF, 2, 8, 300, 9, True, 0),
               (BF, 2, 65, 144, 31, True, 4), (BF, 3, 8, 144, 3, False, 4)]  # the last two: C % 8 == 0 through a view 8 bytes off 16


def _conv(dev, case, kind):
    inp = make_conv(case, kind)
    check_conv(case, kind, inp, run_conv(dev, case, inp))


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", CONV_SIZES, ids=_id)
def test_conv_pair_kernel_sizes(dev, case, kind):
    """K <= 8: the 8-tap instantiation, above: the 32-tap one (taps k >= K are zero weights); bias NULL and given"""
    _conv(dev, case, kind)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", CONV_SEAMS, ids=_id)
def test_conv_pair_kernel_time_seams(dev, case, kind):
    """T around the 16-step thread group and the 32-step workgroup; T shorter than the halo"""
    _conv(dev, case, kind)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", CONV_SLABS, ids=_id)
def test_conv_pair_kernel_channel_slabs(dev, case, kind):
    """one 16-byte piece, a partial slab, an exact slab, a slab plus one piece, two slabs plus a piece"""
    _conv(dev, case, kind)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", CONV_SCALAR, ids=_id)
def test_conv_scalar_kernels(dev, case, kind):
    """f32; bf16 with C % 8 != 0; bf16 off 16 bytes (the tile kernel refuses, the scalar one must give the same).  Block widths 64, 128, 256;
    T across the DW_TT = 8 steps of a block"""
    _conv(dev, case, kind)


# ------------------------------------------------------------------------------------------------------------- weight gradient
def make_wgrad(case, kind, salt=0):
    dtype, B, T, C, Kk, dbias = case[:6]
    g = gen(12, B, T, C, Kk, dbias, kind == "exact", salt)
    return dict(x=acts(g, kind, (B, T, C), dtype), dy=grads(g, kind, (B, T, C), dtype), dw0=lattice(g, (Kk, C), 0.25, 2.0),
                db0=lattice(g, (C,), 0.25, 2.0) if dbias else None)


def run_wgrad(dev, case, inp):
    dtype, B, T, C, Kk, dbias, mode, off = case
    x, dy, dw, db = put(inp["x"], dev, off), put(inp["dy"], dev, off), dev_(inp["dw0"], dev), dev_(inp["db0"], dev)
    need = ws_size(B, T, C, Kk)
    ws = nan_ws(dev, need)
    L = K._L()
    if mode == "direct":
        K.check(L.tfasr_dwconv_bwd_weight(K._p(x), K._p(dy), K._p(dw), K._p(db), B, T, C, Kk, K._dt(x), K._stream()), "dwconv_bwd_weight")
    else:
        wp, nb = (None, 0) if mode == "null" else (K._p(ws), need - 1 if mode == "short" else need)
        K.check(L.tfasr_dwconv_bwd_weight_ws(K._p(x), K._p(dy), K._p(dw), K._p(db), B, T, C, Kk, K._dt(x), wp, nb, K._stream()), "dwconv_bwd_weight_ws")
    return dict(dw=dw.cpu(), dbias=None if db is None else db.cpu(), tile_route=bool((~torch.isnan(ws)).any()))


def check_wgrad(case, kind, inp, out):
    r = DO.dwconv_bwd_weight(inp["x"], inp["dy"], inp["dw0"].shape[0])
    same(kind, "dw", out["dw"], r["dw"] + inp["dw0"].double(), r["M_dw"] + inp["dw0"].double().abs(), k=K_SUM)
    assert (out["dbias"] is None) == (inp["db0"] is None)
    if inp["db0"] is not None:
        same(kind, "dbias", out["dbias"], r["dbias"] + inp["db0"].double(), r["M_dbias"] + inp["db0"].double().abs(), k=K_SUM)


# (dtype, B, T, C, K, dbias, workspace: "ws" | "short" (one byte) | "null" | "direct" (tfasr_dwconv_bwd_weight), elements off 16 bytes)
WGRAD_TILE = ([(BF, 2, 65, 264, Kk, Kk != 7, "ws", 0) for Kk in (3, 5, 7, 15, 31, 32)]
              + [(BF, 3, T, 8, 31, False, "ws", 0) for T in (1, 63, 64, 130)] + [(BF, 2, T, 144, 5, True, "ws", 0) for T in (1, 63, 64, 65, 130)]
              + [(BF, 2, 65, 520, 15, True, "ws", 0)]
              # B * ceil(T / 64) partial slabs per channel slab against the 16 slices: 16 (one each), 18 (two each, slices 9.. empty),
              # 63 (four each: the unrolled loop alone), 80 (five each: the unrolled loop and its tail)
              + [(BF, 8, 128, 8, 3, True, "ws", 0), (BF, 6, 130, 8, 7, True, "ws", 0), (BF, 9, 385, 8, 3, True, "ws", 0), (BF, 10, 450, 8, 5, False, "ws", 0)])
WGRAD_FALLBACK = ([(BF, 2, 65, 144, Kk, True, "ws", 0) for Kk in (1, 8, 9)]  # no tile instantiation
                  + [(BF, 2, 65, 144, 31, True, mode, 0) for mode in ("short", "null", "direct")] + [(BF, 3, 130, 264, 5, False, "short", 0)]
                  + [(F32, 2, 65, 77, 5, True, "ws", 0), (F32, 3, 130, 300, 32, False, "null", 0), (F32, 2, 9, 40, 1, True, "ws", 0)]
                  + [(BF, 2, 65, 100, 31, True, "ws", 0), (BF, 3, 64, 77, 5, False, "ws", 0), (BF, 2, 65, 144, 31, True, "ws", 4)])


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", WGRAD_TILE, ids=_id)
def test_weight_gradient_tile_route(dev, case, kind):
    """tfasr_dwconv_bwd_weight_ws: partial slabs into a NaN workspace, reduced in 16 slices, ADDED to non-zero dw / dbias; dbias NULL"""
    inp = make_wgrad(case, kind)
    out = run_wgrad(dev, case, inp)
    assert out["tile_route"], "the workspace was not written: the fallback ran"
    check_wgrad(case, kind, inp, out)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", WGRAD_FALLBACK, ids=_id)
def test_weight_gradient_fallback(dev, case, kind):
    """the scalar kernel (f32 atomics) wherever the tile route does not apply: the same results, and the NaN workspace is neither read nor
    written"""
    inp = make_wgrad(case, kind)
    out = run_wgrad(dev, case, inp)
    assert not out["tile_route"], "the workspace was written: the tile route ran"
    check_wgrad(case, kind, inp, out)


def run_many(dev, case, inps, n_arg=None, ws_bytes=None):
    dtype, n, B, T, C, Kk = case
    xs, dys = [put(i["x"], dev) for i in inps], [put(i["dy"], dev) for i in inps]
    dws, dbs = [dev_(i["dw0"], dev) for i in inps], [dev_(i["db0"], dev) for i in inps]
    need = n * ws_size(B, T, C, Kk)
    ws = nan_ws(dev, need)
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    st = K._L().tfasr_dwconv_bwd_weight_many(arr(xs), arr(dys), arr(dws), arr(dbs) if any(d is not None for d in dbs) else None, n_arg or n, B, T, C, Kk,
                                             K._dt(xs[0]), K._p(ws), need if ws_bytes is None else ws_bytes, K._stream())
    return st, dict(dw=[d.cpu() for d in dws], dbias=[None if d is None else d.cpu() for d in dbs], tile_route=bool((~torch.isnan(ws)).any()))


def make_many(case, kind):
    dtype, n, B, T, C, Kk = case
    # every product its own data (a swapped product index fails); dbias entries NULL and non-NULL mixed (all NULL for one case: the array itself NULL)
    return [make_wgrad((dtype, B, T, C, Kk, (m % 3 != 1) and not (n == 2 and C == 264)), kind, salt=m + 1) for m in range(n)]


def check_many(case, kind, inps, out):
    for m, inp in enumerate(inps):
        check_wgrad(case, kind, inp, dict(dw=out["dw"][m], dbias=out["dbias"][m]))


# (dtype, products, B, T, C, K)
MANY_CASES = [(BF, 1, 1, 70, 8, 5), (BF, 2, 2, 70, 264, 31), (BF, 5, 3, 70, 8, 31), (BF, 32, 2, 70, 8, 5), (BF, 5, 2, 70, 264, 5)]
MANY_FALLBACK = [(BF, 3, 2, 70, 8, 8), (F32, 3, 2, 70, 8, 5)]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", MANY_CASES, ids=_id)
def test_weight_gradient_of_many_products(dev, case, kind):
    """tfasr_dwconv_bwd_weight_many: blockIdx.z = product * B + utterance, partial slabs product-major, 16 reduce slices per product"""
    inps = make_many(case, kind)
    st, out = run_many(dev, case, inps)
    assert st == 0 and out["tile_route"]
    check_many(case, kind, inps, out)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", MANY_FALLBACK + [(BF, 2, 2, 70, 8, 5)], ids=_id)
def test_weight_gradient_of_many_falls_back_one_by_one(dev, case, kind):
    """K without a tile instantiation, f32, and a workspace one byte short (the last case): product by product through the scalar kernel"""
    inps = make_many(case, kind)
    st, out = run_many(dev, case, inps, ws_bytes=None if case in MANY_FALLBACK else case[1] * ws_size(*case[2:]) - 1)
    assert st == 0 and not out["tile_route"]
    check_many(case, kind, inps, out)


# ------------------------------------------------------------------------------------------------- forward with statistics
def check_stats(kind, y_gpu, st_gpu, st0, ncopy):
    """the statistics of the bf16 y the GPU stored: every copy against the per-copy oracle, and their sum"""
    r = DO.bn_stats_copies(y_gpu, ncopy, 2 * TGD)
    st0 = st0.double()
    same(kind, "stats per copy", st_gpu, r["stats"] + st0, r["M_stats"] + st0.abs(), k=K_SUM)
    t = DO.bn_stats_of(y_gpu)
    same(kind, "stats", st_gpu.double().sum(0).float() if kind == "exact" else st_gpu.double().sum(0), t["stats"] + st0.sum(0), t["M_stats"] + st0.abs().sum(0), k=K_SUM)


def make_fwd_stats(case, kind):
    B, T, C, Kk, ncopy, bias = case
    g = gen(13, B, T, C, Kk, ncopy, kind == "exact")
    w, b = taps(g, kind, Kk, C, bias)
    return dict(x=acts(g, kind, (B, T, C), BF), w=w, bias=b, st0=lattice(g, (ncopy, 2 * C), 0.25, 2.0))


def run_fwd_stats(dev, case, inp):
    B, T, C, Kk, ncopy, bias = case
    x, w, b, st = put(inp["x"], dev), dev_(inp["w"], dev), dev_(inp["bias"], dev), dev_(inp["st0"], dev)
    y = Out(dev, (B, T, C), BF)
    K.check(K._L().tfasr_dwconv_fwd_stats(K._p(x), K._p(w), K._p(b), K._p(y.v), K._p(st), ncopy, B, T, C, Kk, K._dt(x), K._stream()), "dwconv_fwd_stats")
    return dict(y=y.done("y"), stats=st.cpu())


def check_fwd_stats(case, kind, inp, out):
    f = DO.dwconv_fwd(inp["x"], inp["w"], inp["bias"])
    same(kind, "y", out["y"], f["y"], f["M_y"])
    check_stats(kind, out["y"], out["stats"], inp["st0"], case[4])


# (B, T, C, K, ncopy, bias): T with a partial last tile of 32 (rows >= T must not enter the sums)
FWD_STATS_CASES = [(3, 33, 8, 5, 1, True), (2, 70, 264, 5, 3, False), (3, 70, 144, 5, 8, True), (3, 33, 264, 31, 1, False), (2, 70, 8, 31, 3, True),
                   (3, 97, 520, 31, 8, True), (2, 17, 144, 8, 3, True), (2, 17, 144, 9, 3, True)]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", FWD_STATS_CASES, ids=_id)
def test_forward_with_statistics(dev, case, kind):
    """tfasr_dwconv_fwd_stats: sums of the bf16-rounded y, ADDED into copy (time tile + utterance) % ncopy of non-zero statistics"""
    inp = make_fwd_stats(case, kind)
    check_fwd_stats(case, kind, inp, run_fwd_stats(dev, case, inp))


def make_gin(case, kind):
    B, T, C, Kk, ncopy, bias = case
    g = gen(14, B, T, C, Kk, ncopy, kind == "exact")
    w, b = taps(g, kind, Kk, C, bias)
    return dict(glu_x=gated(g, kind, (B, T, C), BF), w=w, bias=b, st0=lattice(g, (ncopy, 2 * C), 0.25, 2.0))


def run_gin(dev, case, inp):
    B, T, C, Kk, ncopy, bias = case
    x, w, b, st = put(inp["glu_x"], dev), dev_(inp["w"], dev), dev_(inp["bias"], dev), dev_(inp["st0"], dev)
    gt, y = Out(dev, (B, T, C), BF), Out(dev, (B, T, C), BF)
    K.check(K._L().tfasr_glu_dwconv_fwd_stats(K._p(x), K._p(gt.v), K._p(w), K._p(b), K._p(y.v), K._p(st), ncopy, B, T, C, Kk, K._dt(x), K._stream()),
            "glu_dwconv_fwd_stats")
    return dict(g=gt.done("g"), y=y.done("y"), stats=st.cpu())


def check_gin(case, kind, inp, out):
    r = DO.glu_fwd(inp["glu_x"])
    same(kind, "g", out["g"], r["g"], r["M_g"])
    f = DO.dwconv_fwd(out["g"], inp["w"], inp["bias"])  # from the g the GPU stored
    same(kind, "y", out["y"], f["y"], f["M_y"])
    check_stats(kind, out["y"], out["stats"], inp["st0"], case[4])


GIN_CASES = [(2, 17, 144, 9, 1, True), (3, 33, 264, 15, 3, False), (2, 65, 520, 32, 8, True), (3, 33, 144, 32, 3, True), (2, 33, 520, 9, 8, False),
             (2, 65, 264, 15, 1, True)]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", GIN_CASES, ids=_id)
def test_gated_forward_with_statistics(dev, case, kind):
    """tfasr_glu_dwconv_fwd_stats: g = a sigmoid(b) rounded to bf16 on its way into LDS; the halo rows are gated by two workgroups and
    stored by their owner only (g, NaN before, equals the reference everywhere and its guards are unchanged)"""
    inp = make_gin(case, kind)
    check_gin(case, kind, inp, run_gin(dev, case, inp))


# -------------------------------------------------------------------------------------- data gradient + GLU backward (+ BatchNorm)
def make_bwd_glu(case, kind):
    B, T, C, Kk = case
    g = gen(15, B, T, C, Kk, kind == "exact")
    return dict(dy=grads(g, kind, (B, T, C), BF), w=taps(g, kind, Kk, C, False)[0], glu_x=gated(g, kind, (B, T, C), BF))


def run_bwd_glu(dev, case, inp):
    B, T, C, Kk = case
    dy, w, x = put(inp["dy"], dev), dev_(inp["w"], dev), put(inp["glu_x"], dev)
    d = Out(dev, (B, T, 2 * C), BF)
    K.check(K._L().tfasr_dwconv_bwd_data_glu(K._p(dy), K._p(w), K._p(x), K._p(d.v), B, T, C, Kk, K._dt(dy), K._stream()), "dwconv_bwd_data_glu")
    return dict(dglu=d.done("dglu"))


def check_bwd_glu(case, kind, inp, out, dy=None):
    b = DO.dwconv_bwd_data(inp["dy"] if dy is None else dy, inp["w"])  # (dx stays in float32 registers: no rounding in between)
    r = DO.glu_bwd(inp["glu_x"], b["dx"], b["M_dx"])
    same(kind, "dglu", out["dglu"], r["d"], r["M_d"])


BWD_GLU_CASES = [(2, 1, 8, 5), (3, 17, 264, 31), (2, 33, 520, 32), (2, 17, 520, 5), (3, 33, 8, 31), (2, 1, 264, 32), (2, 65, 144, 15)]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", BWD_GLU_CASES, ids=_id)
def test_data_gradient_with_glu_backward(dev, case, kind):
    """tfasr_dwconv_bwd_data_glu: the a | b rows are prefetched with the row index clamped to T - 1 (the NaN guard behind the GLU input is
    never read into a result) and the last tile stores nothing past T (guards of dglu unchanged)"""
    inp = make_bwd_glu(case, kind)
    check_bwd_glu(case, kind, inp, run_bwd_glu(dev, case, inp))


def make_bnin(case):
    B, T, C, Kk, copies, with_grads = case
    g = gen(16, B, T, C, Kk, copies, with_grads)
    bn_x = gauss(g, (B, T, C), BF)
    fin = NO.bn_finalize(NO.bn_moments(bn_x)["stats"], B * T, torch.randn(C, generator=g), torch.randn(C, generator=g))["fin"].float()
    return dict(bn_x=bn_x, dsw=torch.randn(B, T, C, generator=g).to(BF), fin=fin, bstats=lattice(g, (copies, 2 * C), 0.125, 4.0), count=float(B * T),
                dg0=lattice(g, (C,), 0.25, 2.0) if with_grads else None, db0=lattice(g, (C,), 0.25, 2.0) if with_grads else None,
                w=torch.randn(Kk, C, generator=g) * 0.5, glu_x=gauss(g, (B, T, 2 * C), BF), gscale=0.5)


def run_bnin(dev, case, inp):
    B, T, C, Kk, copies, with_grads = case
    bn_x, dsw, x = put(inp["bn_x"], dev), put(inp["dsw"], dev), put(inp["glu_x"], dev)
    fin, bst, w, dg, db = (dev_(inp[k], dev) for k in ("fin", "bstats", "w", "dg0", "db0"))
    dcv, d = Out(dev, (B, T, C), BF), Out(dev, (B, T, 2 * C), BF)
    K.check(K._L().tfasr_bn_dwconv_bwd_data_glu(K._p(bn_x), K._p(dsw), K._p(fin), K._p(bst), copies, inp["count"], K._p(dg), K._p(db), inp["gscale"], K._p(dcv.v),
                                                K._p(w), K._p(x), K._p(d.v), B, T, C, Kk, K._dt(bn_x), K._stream()), "bn_dwconv_bwd_data_glu")
    return dict(dcv=dcv.done("dcv"), dglu=d.done("dglu"), dgamma=None if dg is None else dg.cpu(), dbeta=None if db is None else db.cpu())


def check_bnin(case, inp, out):
    C = case[2]
    p = DO.bn_bwd_prologue(inp["bn_x"], inp["dsw"], inp["fin"], inp["bstats"], inp["count"])
    held("dcv", out["dcv"], p["dcv"], p["M_dcv"], bf16=True)
    check_bwd_glu(case[:4], "random", inp, out, dy=out["dcv"])  # from the dcv the GPU stored
    assert (out["dgamma"] is None) == (inp["dg0"] is None) and (out["dbeta"] is None) == (inp["db0"] is None)
    if inp["dg0"] is not None:  # (the sums are lattice values: exact)
        bits_equal("dbeta", out["dbeta"], inp["db0"].double() + inp["gscale"] * p["bsum"][:C])
        bits_equal("dgamma", out["dgamma"], inp["dg0"].double() + inp["gscale"] * p["bsum"][C:])


# (B, T, C, K, copies of bstats, dgamma / dbeta given)
BNIN_CASES = [(2, 17, 144, 31, 1, True), (3, 33, 264, 32, 4, True), (2, 40, 520, 31, 8, True), (2, 33, 144, 5, 4, False), (2, 17, 264, 31, 8, False),
              (3, 65, 520, 15, 1, False)]


@pytest.mark.parametrize("case", BNIN_CASES, ids=_id)
def test_batchnorm_backward_data_gradient_glu_backward(dev, case):
    """tfasr_bn_dwconv_bwd_data_glu: fin and bstats (lattice values, so that dgamma / dbeta += grad_scale * the sum over the copies is
    exact) chosen here; dcv against norm_oracle.bn_bwd_apply with swish, dglu from the dcv the kernel stored"""
    inp = make_bnin(case)
    check_bnin(case, inp, run_bnin(dev, case, inp))


# --------------------------------------------------------------------------------------------------------------------------- GLU
def make_glu(case, kind):
    dtype, rows, C = case
    g = gen(17, rows, C, kind == "exact")
    return dict(x=gated(g, kind, (rows, C), dtype), dg=grads(g, kind, (rows, C), dtype))


def run_glu(dev, case, inp):
    dtype, rows, C = case
    x, dg = put(inp["x"], dev), put(inp["dg"], dev)
    gt, d = Out(dev, (rows, C), dtype), Out(dev, (rows, 2 * C), dtype)
    K.check(K._L().tfasr_glu_fwd(K._p(x), K._p(gt.v), rows, C, K._dt(x), K._stream()), "glu_fwd")
    K.check(K._L().tfasr_glu_bwd(K._p(x), K._p(dg), K._p(d.v), rows, C, K._dt(x), K._stream()), "glu_bwd")
    return dict(g=gt.done("g"), d=d.done("d"))


def check_glu(case, kind, inp, out):
    f, b = DO.glu_fwd(inp["x"]), DO.glu_bwd(inp["x"], inp["dg"])
    if kind == "exact" and case[0] == F32:  # (1 / (1 + exp(-0)) through v_rcp_f32 may be an ulp off 1/2 in float32: bounds, not bits)
        kind = "random"
    same(kind, "g", out["g"], f["g"], f["M_g"])
    same(kind, "d", out["d"], b["d"], b["M_d"])


GLU_SMALL = [(dt, rows, C) for dt in (BF, F32) for rows, C in ((1, 8), (37, 144), (5, 264))]
GLU_BIG = [(dt, 1025, 8200) for dt in (BF, F32)]
assert 1025 * 8200 // 8 > GLU_PASS


@pytest.mark.parametrize("case,kind", [(c, k) for c in GLU_SMALL for k in ("exact", "random")] + [(c, "random") for c in GLU_BIG], ids=_id)
def test_glu(dev, case, kind):
    """tfasr_glu_fwd / tfasr_glu_bwd: below one trip of the grid-stride loop, and past it (rows C / 8 > 256 * 16 * 256 pieces)"""
    inp = make_glu(case, kind)
    check_glu(case, kind, inp, run_glu(dev, case, inp))


# ------------------------------------------------------------------------------------------------------------------ status codes
def test_status_codes(dev):
    """the documented INVALID_VALUE / UNSUPPORTED, and nothing written"""
    L, s = K._L(), K._stream()
    B, T, C, Kk = 2, 17, 16, 5
    BFI, F32I = K._dt(torch.empty(0, dtype=BF)), K._dt(torch.empty(0, dtype=F32))
    x, x2 = torch.zeros(B, T, 104, dtype=BF, device=dev), torch.zeros(B, T, 208, dtype=BF, device=dev)   # (room for C = 100 and f32 at C = 16)
    w, fin = torch.zeros(33, 104, device=dev), torch.ones(4 * 104, device=dev)
    outs = [Out(dev, (B, T, 208), BF) for _ in range(3)]
    y, y2, y3 = (o.v for o in outs)
    f = [Out(dev, (34 * 104,), F32) for _ in range(3)]
    dw, db, st = (o.v for o in f)
    p = K._p
    assert L.tfasr_dwconv_fwd(p(x), p(w), None, p(y), B, T, C, 33, BFI, s) == INVALID
    assert L.tfasr_dwconv_bwd_data(p(x), p(w), p(y), B, T, C, 33, BFI, s) == INVALID
    assert L.tfasr_dwconv_bwd_weight(p(x), p(x), p(dw), p(db), B, T, C, 33, BFI, s) == INVALID
    assert L.tfasr_dwconv_bwd_weight_ws(p(x), p(x), p(dw), p(db), B, T, C, 33, BFI, p(st), 4 * st.numel(), s) == INVALID
    arr = lambda t, n: (ctypes.c_void_p * n)(*[t.data_ptr()] * n)  # noqa: E731
    assert L.tfasr_dwconv_bwd_weight_many(arr(x, 33), arr(x, 33), arr(dw, 33), None, 33, B, T, C, Kk, BFI, p(st), 4 * st.numel(), s) == INVALID
    assert L.tfasr_dwconv_bwd_weight_many(arr(x, 2), arr(x, 2), arr(dw, 2), None, 2, B, T, C, 33, BFI, p(st), 4 * st.numel(), s) == INVALID
    assert L.tfasr_glu_fwd(p(x2), p(y), B * T, 100, BFI, s) == INVALID
    assert L.tfasr_glu_bwd(p(x2), p(x), p(y), B * T, 100, BFI, s) == INVALID
    for Cc, kk, dt in ((C, 33, BFI), (C, Kk, F32I), (100, Kk, BFI)):  # K > 32, not bf16, C % 8 != 0: the fused entries refuse
        assert L.tfasr_dwconv_fwd_stats(p(x), p(w), None, p(y), p(st), 1, B, T, Cc, kk, dt, s) == UNSUPPORTED
        assert L.tfasr_glu_dwconv_fwd_stats(p(x2), p(y2), p(w), None, p(y), p(st), 1, B, T, Cc, max(kk, 9), dt, s) == UNSUPPORTED
        assert L.tfasr_dwconv_bwd_data_glu(p(x), p(w), p(x2), p(y), B, T, Cc, kk, dt, s) == UNSUPPORTED
        assert L.tfasr_bn_dwconv_bwd_data_glu(p(x), p(x), p(fin), p(fin), 1, float(B * T), p(dw), p(db), 1.0, p(y2), p(w), p(x2), p(y3), B, T, Cc, kk, dt, s) == UNSUPPORTED
    xo = x.view(-1)[4:4 + B * T * 2 * C]  # an activation 8 bytes off 16: the fused entries refuse (their callers run the unfused kernels)
    assert xo.data_ptr() % 16 == 8
    assert L.tfasr_dwconv_fwd_stats(p(xo), p(w), None, p(y), p(st), 1, B, T, C, Kk, BFI, s) == UNSUPPORTED
    assert L.tfasr_glu_dwconv_fwd_stats(p(xo), p(y2), p(w), None, p(y), p(st), 1, B, T, C, 9, BFI, s) == UNSUPPORTED
    assert L.tfasr_dwconv_bwd_data_glu(p(xo), p(w), p(x2), p(y), B, T, C, Kk, BFI, s) == UNSUPPORTED
    assert L.tfasr_bn_dwconv_bwd_data_glu(p(xo), p(x), p(fin), p(fin), 1, float(B * T), p(dw), p(db), 1.0, p(y2), p(w), p(x2), p(y3), B, T, C, Kk, BFI, s) == UNSUPPORTED
    assert L.tfasr_glu_dwconv_fwd_stats(p(x2), p(y2), p(w), None, p(y), p(st), 1, B, T, C, 8, BFI, s) == UNSUPPORTED  # K <= 8: no GIN instantiation
    assert L.tfasr_dwconv_fwd_stats(p(x), p(w), None, p(y), p(st), 0, B, T, C, Kk, BFI, s) == INVALID
    assert L.tfasr_bn_dwconv_bwd_data_glu(p(x), p(x), p(fin), p(fin), 0, float(B * T), None, None, 1.0, p(y2), p(w), p(x2), p(y3), B, T, C, Kk, BFI, s) == INVALID
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs + f), "a refused call wrote to an output"
