"""Every entry point and launch branch of csrc/conv2d.hip against the float64 restatements of tests/subsampling_oracle.py, in the method of
tests/test_norm_gpu.py (its `hold` / `exact` are used as they are).

Inputs are rounded to the storage type first and the reference is computed from the rounded values.  Every fin, bstats, gram and pbuf a
kernel consumes is chosen by the TEST from the oracle (never the output of another GPU kernel).  Outputs are pre-filled with NaN; sums
that the kernels ADD to their destination start from a lattice value.  Every comparison prints max |gpu - ref| / bound before it asserts.

Exact cases (indexing): x a small integer in [-2, 2], taps and bias multiples of 1/2 in [-1, 1], gradients small integers: every product
and every sum is exact in float32 in any order (and fits bf16 where the output is bf16), so the output must equal the float64 result bit
for bit: one lost, doubled or misplaced position fails.
Random cases (numerics): log-mel like features (mean -6, std 2.5), with the constants of the norm suite on the sum of |term|:
    an element               |gpu - ref| <= 2^-20 M  (+ 2^-8 |ref| for a bf16 output)
    a sum over positions     |gpu - ref| <= 2^-18 sum |term|
Each route is bounded by the terms IT sums in float32 (subsampling_oracle.bn0_backward_bounds): the two-pass dw on sum |p_k| M_d, the
one-pass pbuf on sum |p_k| M_dz, tfasr_conv1_bn_bwd_finalize by propagating the pbuf / bstats the test supplied: 2^-22 of its terms.
A quantity the kernels recompute counts by the terms it is formed from (z: nine products and the bias; swish' = s + s u (1 - s): two
terms, the norm suite's treatment of ACT_SWISH).  swish / swish' run on the fast exponential and the hardware reciprocal; the ratios
measured on the MI355X are in profiles/conv2d_parity.json: all stayed inside these constants, none was raised.
Sparse-gradient cases: random arithmetic, dy non-zero at a handful of positions (first / last t and f, both parities, the last sample, a
row of a second trip), NaN in every halo / past-the-edge slot of the S-layout dy: the bound is then a few terms wide
(test_subsampling_oracle.py shows it sees one lost or doubled position) and a kernel that reads a slot it must not read returns NaN.

Entry point                        kernels / branches                                                     test
tfasr_conv1_fwd, _fwd_s2d          conv1_fwd_rows_kernel (C = 256, F0 <= 258): F1 < 8 sub-lanes, full     test_conv1_forward_exact, _random
                                   LDS rows, > 8192 rows; conv1_fwd_kernel: C = 256 at F0 = 259, C = 8 /
                                   40 / 144, rounded grid past one pass, bias NULL
tfasr_conv1_bwd_weight, _s2d       conv1_bwd_weight_rows_kernel: 1 row, > 1024 rows;                      test_conv1_weight_gradient_exact, _random
                                   conv1_bwd_weight_kernel<., 32>: C = 8 / 144 / 248, past 1024 blocks, db NULL
tfasr_conv1_stats                  conv1_bn_kernel<., 0, 8>                                               test_conv1_statistics_exact, _random
tfasr_conv1_bn_apply_s2d           conv1_bn_kernel<., 1, 8> (+ tfasr_halo_zero, tfasr_s2d_edge_zero)      test_conv1_bn_apply
tfasr_conv1_bn_bwd_stats_s2d,      conv1_bn_kernel<., 2 | 3 | 4, 4>: C = 8 (more sub-lanes than F1), 144   test_conv1_bn_backward[random | sparse]
  _bwd_apply_s2d, _bwd_onepass_s2d (idle threads), 256; < 64 rows; two trips of every block
tfasr_conv1_gram                   conv1_gram_kernel: < 6 rows, rows % 6 != 0, > 6 x 1024 rows              test_conv1_gram_exact
tfasr_conv1_stats_from_gram        conv1_stats_from_gram_kernel: C = 8, 256, 264 (two blocks), bias NULL   test_conv1_statistics_from_gram
tfasr_conv1_bn_bwd_finalize        conv1_bn_bwd_finalize_kernel: the same, db NULL, count != N (a shard)   test_conv1_bn_backward_finalize, ..._of_two_shards
tfasr_halo_zero                    halo_zero_kernel: W = C, W = 4C, past one flat_grid pass                test_halo_and_edge_zero
tfasr_s2d_edge_zero                s2d_edge_zero_kernel: odd-odd, odd-even, even-odd; even-even returns    test_halo_and_edge_zero
tfasr_im2col_3x3s2, _col2im_3x3s2  im2col_kernel, col2im_kernel: odd / even, T1 = 1, F1 = 1, past one pass test_im2col_and_col2im_exact
(every entry point)                INVALID_VALUE before any launch                                        test_refusals
conv2 through the S layout         ConformerTransducer._seg_tables: forward, data and weight gradients     test_conv2_through_the_s_layout"""
import functools

import pytest
import torch

import subsampling_oracle as SO
from subsampling_oracle import K_DOUBLE, K_FINALIZE, K_SUM
from tensorflowasr_amd import kernels as K
from test_norm_gpu import exact, hold

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
DT = [F32, BF]

# What one pass of each grid-stride loop covers, from the launch arithmetic of csrc/conv2d.hip (past it, a thread makes its second trip).
FWD_ROWS_PASS = 8192                 # conv1_fwd_rows_kernel, conv1_bn_kernel<., 1, .>: grid = min(B T1, 8192), one (b, t) row per block and trip
BWD_ROWS_PASS = 1024                 # conv1_bwd_weight_rows_kernel: grid = min(B T1, 1024)
FLAT_PASS = 256 * 32 * 256           # flat_grid(): <= 256 * 32 blocks x 256 threads, one 8-element group per thread and trip
BWD_FLAT_CAP = 1024 * 64             # conv1_bwd_weight_kernel: grid = min(positions / 64 + 1, 1024) blocks of 4 waves x 2 positions: 8 trips each
#                                      from 64 positions on, and the cap of 1024 blocks from 1024 x 64 positions on
GRAM_PASS = 6 * 1024                 # conv1_gram_kernel: grid = min(ceil(B T1 / 6), 1024) blocks of 6 rows


def flat_fwd_pass(C):
    """conv1_fwd_kernel: flat_grid() rounded UP to a multiple of C / 8 when 256 % (C / 8) != 0, x 256 threads (8-channel groups)"""
    c8 = C // 8
    return (8192 if 256 % c8 == 0 else -(-8192 // c8) * c8) * 256


def _id(v):
    return {BF: "bf16", F32: "f32"}.get(v) if isinstance(v, torch.dtype) else None


def just_past(n, one_pass):
    """more than one pass, by under 1 %"""
    return one_pass < n <= one_pass * 1.01


def ints(g, shape, lim, dtype=F32):
    return torch.randint(-lim, lim + 1, shape, generator=g).to(dtype)


def halves(g, shape, lim=1.0):
    n = int(round(lim * 2))
    return torch.randint(-n, n + 1, shape, generator=g).float() * 0.5


def nans(dev, *shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def s_shape(B, T0, F0, C):
    T1, F1, T2, F2 = SO.dims(T0, F0)
    return (B, T2 + 1, F2 + 1, 2, 2, C)


def check_s_output(what, y, dense_ref, check):
    """an S-layout output: its elements against the dense reference (`check(what, got, ref)`), every other slot still NaN"""
    B, T1, F1, C = dense_ref.shape
    yc = y.cpu().reshape(B, (T1 + 1) // 2 + 1, (F1 + 1) // 2 + 1, 2, 2, C)
    check(what, SO.from_s2d(yc, T1, F1), dense_ref)
    assert bool(torch.isnan(yc[~SO.valid_mask(B, T1, F1)]).all()), f"{what}: a halo / past-the-edge slot was written"


# ----------------------------------------------------------------------------------------------------------------- conv1 forward
FWD_CASES = {                                   # B, T0, F0, C
    "rows_F1_below_8_sublanes": (2, 5, 7, 256),
    "rows_full_lds": (1, 3, 258, 256),          # F0 + 2 = 260: the LDS rows are full, 17 trips of the 8 f sub-lanes (F1 = 129)
    "rows_past_8192": (3, 5463, 3, 256),
    "flat_c256_F0_259": (1, 4, 259, 256),       # the other side of the `C == 256 && F0 + 2 <= 260` switch
    "flat_c144_one": (2, 1, 1, 144),
    "flat_c144": (2, 6, 8, 144),
    "flat_c40": (3, 7, 5, 40),
    "flat_c8": (2, 9, 4, 8),
    "flat_c8_T0_1": (1, 1, 6, 8),
    "flat_c144_past_rounded_grid": (2, 2336, 100, 144),   # 8192 -> 8208 blocks: only the rounding keeps a thread on its channel group
    "flat_c40_past_rounded_grid": (2, 8392, 100, 40),     # 8192 -> 8195 blocks
}
for _n, (_B, _T0, _F0, _C) in FWD_CASES.items():
    _T1, _F1, _, _ = SO.dims(_T0, _F0)
    if "rows_past" in _n:
        assert just_past(_B * _T1, FWD_ROWS_PASS)
    if "past_rounded" in _n:
        assert just_past(_B * _T1 * _F1 * (_C // 8), flat_fwd_pass(_C)) and flat_fwd_pass(_C) > FLAT_PASS and (FLAT_PASS % (_C // 8)) != 0
    assert ("rows" in _n) == (_C == 256 and _F0 + 2 <= 260)


@functools.lru_cache(maxsize=1)
def fwd_exact_case(name):
    B, T0, F0, C = FWD_CASES[name]
    g = SO.gen(31, B, T0, F0, C)
    x, w, b = ints(g, (B, T0, F0), 2), halves(g, (3, 3, 1, C)), halves(g, (C,))
    return x, w, b, SO.conv1(x, w, b)[0]  # |z| <= 9 * 2 + 1 in steps of 1/2: 8 bits


@pytest.mark.parametrize("name,dtype", [(n, d) for n in FWD_CASES for d in DT], ids=_id)  # (both types of a case share one reference)
def test_conv1_forward_exact(dev, name, dtype):
    """tfasr_conv1_fwd (dense) and tfasr_conv1_fwd_s2d (S layout; the slots that hold no element stay NaN) on the lattice: bit for bit"""
    x, w, b, z = fwd_exact_case(name)
    xd, wd, bd = x.to(dtype).to(dev), w.to(dev), b.to(dev)
    B, T0, F0, C = FWD_CASES[name]
    T1, F1, _, _ = SO.dims(T0, F0)
    y = nans(dev, B, T1, F1, C, dtype=dtype)
    K.check(K._L().tfasr_conv1_fwd(K._p(xd), K._p(wd), K._p(bd), K._p(y), B, T0, F0, C, K._dt(xd), K._stream()), "conv1_fwd")
    exact("y", y, z)
    ys = K.conv1_fwd_s2d(xd, wd, bd, nans(dev, *s_shape(B, T0, F0, C), dtype=dtype))
    check_s_output("y (S layout)", ys, z, exact)
    if name in ("rows_F1_below_8_sublanes", "flat_c144"):  # bias == NULL
        y = nans(dev, B, T1, F1, C, dtype=dtype)
        K.check(K._L().tfasr_conv1_fwd(K._p(xd), K._p(wd), None, K._p(y), B, T0, F0, C, K._dt(xd), K._stream()), "conv1_fwd")
        exact("y without bias", y, z - b.double())


RANDOM_SHAPES = [(3, 37, 80, 256), (2, 21, 17, 144), (2, 6, 259, 256), (3, 10, 9, 8)]


def random_conv1(g, B, T0, F0, C, dtype):
    return SO.logmel_like(g, (B, T0, F0), dtype), torch.randn(3, 3, 1, C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("B,T0,F0,C", RANDOM_SHAPES)
def test_conv1_forward_random(dev, B, T0, F0, C, dtype):
    x, w, b = random_conv1(SO.gen(32, B, T0, F0, C), B, T0, F0, C, dtype)
    z, M = SO.conv1(x, w, b)
    y = K.conv1_fwd(x.to(dev), w.to(dev), b.to(dev))
    hold("y", y, z, M, bf16=dtype == BF)
    ys = K.conv1_fwd_s2d(x.to(dev), w.to(dev), b.to(dev), nans(dev, *s_shape(B, T0, F0, C), dtype=dtype))
    check_s_output("y (S layout)", ys, z, lambda what, got, ref: hold(what, got, ref, M, bf16=dtype == BF))


# --------------------------------------------------------------------------------------------------------- conv1 weight gradient
BWD_W_CASES = {
    "rows_one_row": (1, 1, 9, 256),
    "rows_past_1024": (3, 685, 5, 256),
    "flat_c8": (2, 7, 9, 8),
    "flat_c144": (3, 6, 10, 144),
    "flat_c248": (2, 5, 5, 248),
    "flat_c256_F0_259": (1, 2, 259, 256),
    "flat_8_trips": (5, 15, 409, 8),            # 8200 positions on 129 blocks
    "flat_past_1024_blocks": (4, 80, 819, 144),  # 65 600 positions: the grid is capped
}
assert just_past(3 * 343, BWD_ROWS_PASS) and just_past(4 * 40 * 410, BWD_FLAT_CAP)


def s_gradient(dy_dense, dev):
    """the dense gradient in the S layout, NaN in every slot that holds no element"""
    return SO.to_s2d(dy_dense, fill=NAN).to(dev)


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("name", list(BWD_W_CASES))
def test_conv1_weight_gradient_exact(dev, name, dtype):
    """tfasr_conv1_bwd_weight and _s2d ADD dw / db (db may be NULL); integers: at most 4 positions' worth per term, exact below 2^24"""
    B, T0, F0, C = BWD_W_CASES[name]
    T1, F1, _, _ = SO.dims(T0, F0)
    assert (B * T1 * F1 + 1) * 4 < 2 ** 24
    g = SO.gen(33, B, T0, F0, C)
    x, dy = ints(g, (B, T0, F0), 2, dtype), ints(g, (B, T1, F1, C), 2, dtype)
    dw0, db0 = ints(g, (3, 3, 1, C), 3), ints(g, (C,), 3)
    r = SO.conv1_weight_grad(x, dy)
    dw, db = dw0.to(dev), db0.to(dev)
    K.conv1_bwd_weight(x.to(dev), dy.to(dev), dw, db)
    exact("dw", dw, r["dw"] + dw0.double().reshape(9, C))
    exact("db", db, r["db"] + db0.double())
    dw, db = dw0.to(dev), db0.to(dev)
    K.conv1_bwd_weight_s2d(x.to(dev), s_gradient(dy, dev), dw, db, C)
    exact("dw (S layout)", dw, r["dw"] + dw0.double().reshape(9, C))
    exact("db (S layout)", db, r["db"] + db0.double())
    dw = dw0.to(dev)
    K.conv1_bwd_weight_s2d(x.to(dev), s_gradient(dy, dev), dw, None, C)
    exact("dw (S layout, db NULL)", dw, r["dw"] + dw0.double().reshape(9, C))


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("B,T0,F0,C", RANDOM_SHAPES)
def test_conv1_weight_gradient_random(dev, B, T0, F0, C, dtype):
    g = SO.gen(34, B, T0, F0, C)
    x, _, _ = random_conv1(g, B, T0, F0, C, dtype)
    T1, F1, _, _ = SO.dims(T0, F0)
    dy = (torch.randn(B, T1, F1, C, generator=g) * 0.5).to(dtype)
    r = SO.conv1_weight_grad(x, dy)
    for s2d in (False, True):
        dw, db = torch.full((3, 3, 1, C), 0.5, device=dev), torch.full((C,), -0.25, device=dev)
        if s2d:
            K.conv1_bwd_weight_s2d(x.to(dev), s_gradient(dy, dev), dw, db, C)
        else:
            K.conv1_bwd_weight(x.to(dev), dy.to(dev), dw, db)
        hold(f"dw s2d={s2d}", dw, r["dw"] + 0.5, r["M_dw"] + 0.5, k=K_SUM)
        hold(f"db s2d={s2d}", db, r["db"] - 0.25, r["M_db"] + 0.25, k=K_SUM)


# ----------------------------------------------------------------------------------------------- conv1 statistics, apply, backward
def resident_blocks_at_most():
    p = torch.cuda.get_device_properties(0)
    return p.multi_processor_count * p.max_threads_per_multi_processor // 256


def test_two_trip_case_is_past_two_rounds_of_resident_blocks(dev):
    """the backward grids are min(B T1, max(64, occupancy x CUs)): with 2 x (CUs x threads per CU / 256) + 1 rows every block makes at
    least two trips whatever the occupancy query returned"""
    B, T0, _, _ = SO.BN0_CASES["two_trips"]
    assert B * SO.dims(T0, 9)[0] >= 2 * resident_blocks_at_most() + 1


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("name", list(SO.BN0_CASES))
def test_conv1_statistics_exact(dev, name, dtype):
    """tfasr_conv1_stats ADDS (sum z, sum z^2): z in steps of 1/2, z^2 in steps of 1/4"""
    B, T0, F0, C = SO.BN0_CASES[name]
    T1, F1, _, _ = SO.dims(T0, F0)
    N = B * T1 * F1
    xl, wl = (2, 1.0) if N < 10000 else (1, 0.5)
    assert (N + 1) * 4 * (9 * xl * wl + wl) ** 2 < 2 ** 24
    g = SO.gen(35, B, T0, F0, C)
    x, w, b = ints(g, (B, T0, F0), xl, dtype), halves(g, (3, 3, 1, C), wl), halves(g, (C,), wl)
    st0 = ints(g, (2 * C,), 3)
    st = st0.to(dev)
    K.conv1_stats(x.to(dev), w.to(dev), b.to(dev), st)
    exact("stats", st, SO.stats(SO.conv1(x, w, b)[0])["stats"] + st0.double())


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("name", list(SO.BN0_CASES))
def test_conv1_statistics_random(dev, name, dtype):
    i = SO.bn0_inputs(name, dtype, "random")
    r = SO.stats(*SO.conv1(i["x"], i["w"], i["b"]))
    st = torch.full((2 * i["w"].shape[-1],), 0.5, device=dev)
    K.conv1_stats(i["x"].to(dev), i["w"].to(dev), i["b"].to(dev), st)
    hold("stats", st, r["stats"] + 0.5, r["M_stats"] + 0.5, k=K_SUM)


APPLY_CASES = list(SO.BN0_CASES) + [(3, 5463, 3, 256)]
assert just_past(3 * SO.dims(5463, 3)[0], FWD_ROWS_PASS)


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("name", APPLY_CASES, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_conv1_bn_apply(dev, name, dtype):
    """tfasr_conv1_bn_apply_s2d: the elements against swish(conv1(x) scale + shift), held to 2^-20 M like tfasr_bn_apply_fwd with
    ACT_SWISH; every halo / past-the-edge slot is still NaN.  Then tfasr_halo_zero + tfasr_s2d_edge_zero: those slots exactly 0, nothing else moved."""
    i = SO.bn0_inputs(name, dtype, "random")
    B, T0, F0 = i["x"].shape
    C = i["w"].shape[-1]
    T1, F1, T2, F2 = SO.dims(T0, F0)
    r = SO.bn0_apply(i["x"], i["w"], i["b"], i["fin"])
    y = K.conv1_bn_apply_s2d(i["x"].to(dev), i["w"].to(dev), i["b"].to(dev), i["fin"].to(dev), nans(dev, *s_shape(B, T0, F0, C), dtype=dtype))
    check_s_output("y", y, r["y"], lambda what, got, ref: hold(what, got, ref, r["M_y"], bf16=dtype == BF))
    before = y.clone()
    K.halo_zero(y, B, T2, F2, 4 * C)
    K.s2d_edge_zero(y, B, T1, F1, C)
    valid = SO.valid_mask(B, T1, F1).to(dev)
    assert torch.equal(y[valid], before[valid]) and int((y[~valid] != 0).sum()) == 0 and not bool(torch.isnan(y).any())


@pytest.mark.parametrize("kind", ["random", "sparse"])
@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("name", list(SO.BN0_CASES))
def test_conv1_bn_backward(dev, name, dtype, kind):
    """tfasr_conv1_bn_bwd_stats_s2d, _bwd_apply_s2d (two passes) and _bwd_onepass_s2d, each against the closed form in float64.  The apply
    pass gets bstats the test chose (random: 1.25 x the true sums, so that db is not ~ 0; sparse: the true sums, as in the detection test)."""
    i = SO.bn0_inputs(name, dtype, kind)
    C = i["w"].shape[-1]
    own = SO.bn0_backward(i["x"], i["w"], i["b"], i["fin"], i["dy"], i["count"])["bstats"]
    bs = (own * (1.25 if kind == "random" else 1.0)).float()
    r = SO.bn0_backward(i["x"], i["w"], i["b"], i["fin"], i["dy"], i["count"], bstats=bs)
    bound = SO.bn0_backward_bounds(r)
    x, w, b, fin, dyS = i["x"].to(dev), i["w"].to(dev), i["b"].to(dev), i["fin"].to(dev), s_gradient(i["dy"], dev)
    c0 = 0.5 if kind == "random" else 0.0   # (sparse: the bound is a few terms wide, the destination starts from zero)
    e0 = K_SUM * c0
    bst = torch.full((2 * C,), c0, device=dev)
    K.conv1_bn_bwd_stats_s2d(x, w, b, fin, dyS, bst)
    hold("bstats (two passes)", bst, r["bstats"] + c0, bound["bstats"] + e0, k=1.0)
    dw, db = torch.full((3, 3, 1, C), c0, device=dev), torch.full((C,), c0, device=dev)
    K.conv1_bn_bwd_apply_s2d(x, w, b, fin, bs.to(dev), i["count"], dyS, dw, db)
    hold("dw (two passes)", dw, r["dw"] + c0, bound["dw"] + e0, k=1.0)
    hold("db (two passes)", db, r["db"] + c0, bound["db"] + e0, k=1.0)
    dw = torch.full((3, 3, 1, C), c0, device=dev)
    K.conv1_bn_bwd_apply_s2d(x, w, b, fin, bs.to(dev), i["count"], dyS, dw, None)
    hold("dw (two passes, db NULL)", dw, r["dw"] + c0, bound["dw"] + e0, k=1.0)
    bst, pbuf = torch.full((2 * C,), c0, device=dev), torch.full((10 * C,), c0, device=dev)
    K.conv1_bn_bwd_onepass_s2d(x, w, b, fin, dyS, bst, pbuf)
    hold("bstats (one pass)", bst, r["bstats"] + c0, bound["bstats"] + e0, k=1.0)
    hold("pbuf", pbuf, torch.cat([r["P"].reshape(-1), r["bstats"][:C]]) + c0, bound["pbuf"] + e0, k=1.0)


# -------------------------------------------------------------------------------------------------------------- the Gram route
def gram_copies(g, gm, dev):
    """the 91 numbers spread unevenly over the 8 copies (stride 96) the consumers add up; integers and halves, so the split is exact"""
    cp = torch.zeros(8, 96, dtype=torch.float64)
    cp[1:, :91] = torch.randint(-8, 9, (7, 91), generator=g).double() * 0.5
    cp[0, :91] = gm - cp[1:, :91].sum(0)
    cp[:, 91:] = NAN  # (padding: never read)
    return cp.reshape(-1).to(dev)


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("B,T0,F0", [(1, 9, 11), (2, 13, 8), (3, 4099, 5), (1, 1, 1)])
def test_conv1_gram_exact(dev, B, T0, F0, dtype):
    """tfasr_conv1_gram: the 8 copies add up to G, s, N exactly (integers in double); < 6 rows, rows % 6 != 0, just past 6 x 1024 rows"""
    T1 = SO.dims(T0, F0)[0]
    assert (B, T0) != (3, 4099) or just_past(B * T1, GRAM_PASS)
    x = ints(SO.gen(36, B, T0, F0), (B, T0, F0), 2, dtype)
    gm = K.conv1_gram(x.to(dev), torch.full((K.CONV1_GRAM_DOUBLES,), NAN, dtype=torch.float64, device=dev))
    got = gm.cpu().view(8, 96)[:, :91].sum(0)
    want = SO.gram(x)
    assert torch.equal(got, want), f"{int((got != want).sum())} of 91 differ"
    assert float(got[90]) == B * T1 * SO.dims(T0, F0)[1]


GRAM_CASES = [(8, True), (256, True), (264, True), (256, False)]  # C, with bias


def gram_case(C, with_bias, dtype=F32, B=2):
    i = SO.bn0_inputs((B, 9, 7, C), dtype, "random")
    if not with_bias:
        i["b"] = None
    return i


@pytest.mark.parametrize("C,with_bias", GRAM_CASES)
def test_conv1_statistics_from_gram(dev, C, with_bias):
    """tfasr_conv1_stats_from_gram works in double and rounds once: an ulp of the result + 2^-44 of the terms"""
    i = gram_case(C, with_bias)
    gm = SO.gram(i["x"])
    r = SO.stats_from_gram(gm, i["w"], i["b"])
    st = nans(dev, 2 * C)
    K.conv1_stats_from_gram(gram_copies(SO.gen(37, C), gm, dev), i["w"].to(dev), None if i["b"] is None else i["b"].to(dev), st)
    hold("stats", st, r["stats"], 2.0 ** -23 * r["stats"].abs() + K_DOUBLE * r["M_stats"], k=1.0)


def finalize_inputs(i, whole=None):
    """pbuf = [P | sum dz] and gram of the batch in `i`, bstats (1.25 x) and count of `whole` (default: the same batch), all rounded as stored"""
    own = SO.bn0_backward(i["x"], i["w"], i["b"], i["fin"], i["dy"], i["count"])
    w_ = own if whole is None else whole
    C = own["P"].shape[1]
    return torch.cat([own["P"].reshape(-1), own["bstats"][:C]]).float(), (w_["bstats"] * 1.25).float(), SO.gram(i["x"])


@pytest.mark.parametrize("C,with_bias", GRAM_CASES)
def test_conv1_bn_backward_finalize(dev, C, with_bias):
    """tfasr_conv1_bn_bwd_finalize ADDS dw / db (db may be NULL) from gram, pbuf and bstats the test supplied: 2^-22 of its terms"""
    i = gram_case(C, with_bias)
    g = SO.gen(38, C)
    pbuf, bs, gm = finalize_inputs(i)
    r = SO.bn0_finalize(gm, i["w"], i["b"], i["fin"], bs, i["count"], pbuf)
    dw0, db0 = halves(g, (3, 3, 1, C)), halves(g, (C,))
    bd = None if i["b"] is None else i["b"].to(dev)
    for with_db in (True, False):
        dw, db = dw0.to(dev), db0.to(dev) if with_db else None
        K.conv1_bn_bwd_finalize(gram_copies(g, gm, dev), i["w"].to(dev), bd, i["fin"].to(dev), bs.to(dev), i["count"], pbuf.to(dev), dw, db)
        hold("dw", dw, r["dw"] + dw0.double().reshape(9, C), r["M_dw"] + dw0.abs().double().reshape(9, C), k=K_FINALIZE)
        if with_db:
            hold("db", db, r["db"] + db0.double(), r["M_db"] + db0.abs().double(), k=K_FINALIZE)


def test_conv1_bn_backward_finalize_of_two_shards(dev):
    """data-parallel training: gram and pbuf of HALF the batch with bstats and count of the whole (gram[90] != count).  Each shard against
    the oracle's shard, and the two dw summed against the whole-batch TWO-PASS dw of the oracle; the two db sum to ~ 0, neither is."""
    C = 64
    i = gram_case(C, True, B=4)
    whole = SO.bn0_backward(i["x"], i["w"], i["b"], i["fin"], i["dy"], i["count"])
    bs = whole["bstats"].float()
    ref = SO.bn0_backward(i["x"], i["w"], i["b"], i["fin"], i["dy"], i["count"], bstats=bs)
    dw, db, M_dw, M_db = torch.zeros(9, C, dtype=torch.float64), [], 0.0, 0.0
    for sl in (slice(0, 2), slice(2, 4)):
        sh = SO.bn0_backward(i["x"][sl], i["w"], i["b"], i["fin"], i["dy"][sl], i["count"], i["count"] // 2, bstats=bs)
        pbuf, gm = torch.cat([sh["P"].reshape(-1), sh["bstats"][:C]]).float(), SO.gram(i["x"][sl])
        assert float(gm[90]) * 2 == i["count"]
        r = SO.bn0_finalize(gm, i["w"], i["b"], i["fin"], bs, i["count"], pbuf)
        dwd, dbd = torch.zeros(3, 3, 1, C, device=dev), torch.zeros(C, device=dev)
        K.conv1_bn_bwd_finalize(gram_copies(SO.gen(39), gm, dev), i["w"].to(dev), i["b"].to(dev), i["fin"].to(dev), bs.to(dev), i["count"], pbuf.to(dev), dwd, dbd)
        hold("dw of one shard", dwd, r["dw"], r["M_dw"], k=K_FINALIZE)
        hold("db of one shard", dbd, r["db"], r["M_db"], k=K_FINALIZE)
        assert float(dbd.abs().max()) > 1e-3
        dw += dwd.double().cpu().reshape(9, C)
        db.append(dbd.double().cpu())
        M_dw, M_db = M_dw + r["M_dw"], M_db + r["M_db"]
    # (+ 2^-24: the float32 rounding of the two pbuf the test handed over)
    hold("dw of both shards", dw, ref["dw"], M_dw, k=K_FINALIZE + 2.0 ** -24)
    hold("db of both shards", db[0] + db[1], ref["db"], M_db, k=K_FINALIZE + 2.0 ** -24)


# ------------------------------------------------------------------------------------------------------ halo / edge zero, im2col
ZERO_CASES = [(2, 5, 7, 8), (2, 5, 6, 16), (3, 6, 7, 8), (2, 6, 4, 64), (1, 1, 1, 8)]  # B, T1, F1, C: odd-odd, odd-even, even-odd, even-even


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def halo_check(dev, dtype, B, T2, F2, W):
    """tfasr_halo_zero: row 0 / column 0 of every sample exactly 0, every other bit as it was (all compared on the device)"""
    g = torch.Generator(device=dev).manual_seed(B * 1000 + T2)
    x = (torch.randint(1, 100, (B, T2 + 1, F2 + 1, W), generator=g, device=dev).float() / 8).to(dtype)
    want = x.clone()
    want[:, 0] = 0
    want[:, :, 0] = 0
    K.halo_zero(x, B, T2, F2, W)
    assert torch.equal(bits(x), bits(want)), f"halo_zero W = {W}"


def edge_check(dev, dtype, B, T1, F1, C):
    """tfasr_s2d_edge_zero: the slots past an odd T1 / F1 exactly 0, every other bit as it was - the NaN halo included"""
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    g = torch.Generator(device=dev).manual_seed(B * 1000 + T1)
    x = (torch.randint(1, 100, (B, T2 + 1, F2 + 1, 2, 2, C), generator=g, device=dev).float() / 8).to(dtype)
    x[:, 0] = NAN  # the halo is not this kernel's: NaN must stay
    want = x.clone()
    if T1 & 1:
        want[:, T2, 1:, 1] = 0
    if F1 & 1:
        want[:, 1:, F2, :, 1] = 0
    K.s2d_edge_zero(x, B, T1, F1, C)
    assert torch.equal(bits(x), bits(want)), "s2d_edge_zero"


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("B,T1,F1,C", ZERO_CASES)
def test_halo_and_edge_zero(dev, B, T1, F1, C, dtype):
    for W in (4 * C, C):  # the S layout, and the conv2 output side
        halo_check(dev, dtype, B, (T1 + 1) // 2, (F1 + 1) // 2, W)
    edge_check(dev, dtype, B, T1, F1, C)


def test_halo_and_edge_zero_past_one_pass(dev):
    """thin tensors (F2 = 1), bf16: tfasr_halo_zero visits B (F2 + 1 + T2) W / 8 groups, tfasr_s2d_edge_zero B (2 F2 + 2 T2) C / 8"""
    B, T1, F1, C = 2, 32767, 1, 256
    T2, F2 = (T1 + 1) // 2, 1
    assert just_past(B * (2 * F2 + 2 * T2) * (C // 8), FLAT_PASS)
    edge_check(dev, BF, B, T1, F1, C)
    B, T2, W = 2, 8191, 1024
    assert just_past(B * ((F2 + 1) + T2) * (W // 8), FLAT_PASS)
    halo_check(dev, BF, B, T2, F2, W)


COL_CASES = [(2, 5, 7, 8), (3, 6, 4, 64), (2, 1, 6, 8), (2, 5, 1, 64), (1, 1, 1, 8)]  # B, T1, F1, C
IM2COL_PAST = (8, 22, 662, 64)     # B T2 F2 9 C / 8 groups
COL2IM_PAST = (1, 513, 512, 64)    # B T1 F1 C / 8 groups (bf16 only: dcol is 38 M elements)
assert just_past(8 * 11 * 331 * 9 * 8, FLAT_PASS) and just_past(513 * 512 * 8, FLAT_PASS)


@pytest.mark.parametrize("shape,dtype", [(s, d) for s in COL_CASES for d in DT] + [(IM2COL_PAST, F32), (IM2COL_PAST, BF), (COL2IM_PAST, BF)], ids=_id)
def test_im2col_and_col2im_exact(dev, shape, dtype):
    """copies and sums of at most 4 small integers: bit for bit (past one pass: each kernel at its own shape)"""
    B, T1, F1, C = shape
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    g = SO.gen(40, B, T1, F1, C)
    if shape != COL2IM_PAST:
        x = ints(g, (B, T1, F1, C), 100, dtype)
        col = nans(dev, B * T2 * F2, 9 * C, dtype=dtype)
        K.im2col_3x3s2(x.to(dev), col)
        exact("col", col, SO.im2col(x))
    if shape != IM2COL_PAST:
        dcol = ints(g, (B * T2 * F2, 9 * C), 2, dtype)
        dx = K.col2im_3x3s2(dcol.to(dev), B, T1, F1, C)
        exact("dx", dx, SO.col2im(dcol, B, T1, F1, C))


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    """C % 8 != 0, C > 256 where the kernel holds C channels in one block, count <= 0, a NULL required pointer: INVALID_VALUE before any
    launch, the outputs still NaN"""
    L = K._L()
    p, st = K._p, K._stream
    B, T0, F0 = 2, 5, 6
    x = torch.zeros(B, T0, F0, device=dev)

    def buf(n, dtype=F32):
        return nans(dev, n, dtype=dtype)

    outs = []

    def out(n, dtype=F32):
        outs.append(buf(n, dtype))
        return p(outs[-1])

    big = 4096 * 16
    w, fin, bs, dy, gm, pb = (torch.zeros(big, device=dev) for _ in range(6))
    gm = gm.double()
    calls = []
    for C in (12, 0):
        calls += [L.tfasr_conv1_fwd(p(x), p(w), p(w), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_conv1_fwd_s2d(p(x), p(w), p(w), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_s2d_edge_zero(out(big), B, 3, 3, C, 0, st()),
                  L.tfasr_halo_zero(out(big), B, 2, 2, C, 0, st()),
                  L.tfasr_im2col_3x3s2(p(w), out(big), B, 3, 3, C, 0, st()),
                  L.tfasr_col2im_3x3s2(p(w), out(big), B, 3, 3, C, 0, st())]
    for C in (12, 264):
        calls += [L.tfasr_conv1_bwd_weight(p(x), p(dy), out(big), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_conv1_bwd_weight_s2d(p(x), p(dy), out(big), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_conv1_stats(p(x), p(w), p(w), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_conv1_bn_apply_s2d(p(x), p(w), p(w), p(fin), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_conv1_bn_bwd_stats_s2d(p(x), p(w), p(w), p(fin), p(dy), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_conv1_bn_bwd_apply_s2d(p(x), p(w), p(w), p(fin), p(bs), 10.0, p(dy), out(big), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_conv1_bn_bwd_onepass_s2d(p(x), p(w), p(w), p(fin), p(dy), out(big), out(big), B, T0, F0, C, 0, st())]
    C = 8
    for count in (0.0, -3.0):
        calls += [L.tfasr_conv1_bn_bwd_apply_s2d(p(x), p(w), p(w), p(fin), p(bs), count, p(dy), out(big), out(big), B, T0, F0, C, 0, st()),
                  L.tfasr_conv1_bn_bwd_finalize(p(gm), p(w), p(w), p(fin), p(bs), count, p(pb), out(big), out(big), C, st())]
    calls += [L.tfasr_conv1_fwd(None, p(w), p(w), out(big), B, T0, F0, C, 0, st()),
              L.tfasr_conv1_fwd(p(x), None, p(w), out(big), B, T0, F0, C, 0, st()),
              L.tfasr_conv1_bwd_weight(p(x), None, out(big), out(big), B, T0, F0, C, 0, st()),
              L.tfasr_conv1_bn_apply_s2d(p(x), p(w), p(w), None, out(big), B, T0, F0, C, 0, st()),
              L.tfasr_conv1_bn_bwd_stats_s2d(p(x), p(w), p(w), p(fin), None, out(big), B, T0, F0, C, 0, st()),
              L.tfasr_conv1_bn_bwd_apply_s2d(p(x), p(w), p(w), p(fin), None, 10.0, p(dy), out(big), out(big), B, T0, F0, C, 0, st()),
              L.tfasr_conv1_bn_bwd_onepass_s2d(p(x), p(w), p(w), None, p(dy), out(big), out(big), B, T0, F0, C, 0, st()),
              L.tfasr_conv1_stats_from_gram(None, p(w), p(w), out(big), C, st()),
              L.tfasr_conv1_bn_bwd_finalize(p(gm), p(w), p(w), p(fin), p(bs), 10.0, None, out(big), out(big), C, st()),
              L.tfasr_conv1_fwd(p(x), p(w), p(w), out(big), B, T0, F0, C, 7, st()),                      # no such dtype
              L.tfasr_conv1_fwd(p(x), p(w), p(w), out(big), 0, T0, F0, C, 0, st())]
    torch.cuda.synchronize()
    assert all(s == 1 for s in calls), calls  # TFASR_STATUS_INVALID_VALUE
    assert all(bool(torch.isnan(o).all()) for o in outs)
    assert L.tfasr_conv1_gram(p(x), None, B, T0, F0, 0, st()) == 1 and L.tfasr_conv1_gram(None, p(gm), B, T0, F0, 0, st()) == 1


# ------------------------------------------------------------------------------------------------------- conv2 through the S layout
@pytest.fixture(scope="module")
def seg_model(dev):
    from tensorflowasr_amd import configs
    from tensorflowasr_amd.conformer import ConformerTransducer

    return ConformerTransducer(configs.conformer_s(dropout=0.0, num_blocks=1), dev, dtype=BF, seed=0)


def gemm_close(what, got, ref, dtype, Kdim):
    """the bound of tests/test_gemm_gpu.py: rtol, atol sqrt(K) with (2e-2, 2e-2) for bf16 and (1e-5, 1e-4) for float32"""
    rtol, atol = (2e-2, 2e-2) if dtype == BF else (1e-5, 1e-4)
    got = got.detach().double().cpu().reshape(ref.shape)
    bound = atol * Kdim ** 0.5 + rtol * ref.abs()
    err = (got - ref).abs()
    print(f"{what} ({_id(dtype)}): max |gpu - ref| / bound = {float((err / bound).max()):.3g}")
    assert bool((err <= bound).all()), what


@pytest.mark.parametrize("dtype", DT, ids=_id)
@pytest.mark.parametrize("T1,F1", [(13, 40), (12, 39)])
def test_conv2_through_the_s_layout(dev, seg_model, T1, F1, dtype):
    """ConformerTransducer._seg_tables: the forward 9-segment product, the four parity-block data-gradient products and the nine
    weight-gradient products with column sums, as _subsampling_fwd_s2d / _bwd_s2d launch them (bf16: segmented; float32: plain products),
    against the float64 autograd of the convolution.  The halo of the incoming gradient is zero; only the elements of da1 are compared."""
    B, C = 3, 64
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    g = SO.gen(41, T1, F1)
    x1 = torch.randn(B, T1, F1, C, generator=g).to(dtype)
    W, b = (torch.randn(9 * C, C, generator=g) * 0.1).to(dtype), torch.randn(C, generator=g) * 0.1
    dy = torch.randn(B, T2, F2, C, generator=g).to(dtype)
    r = SO.conv2(x1, W, b, dy)
    shift, blk, fwd, dgrad = seg_model._seg_tables(F2, C)
    rows, slack = B * (T2 + 1) * (F2 + 1), F2 + 2

    def slacked(t, width):  # [rows, width] between `slack` zero rows, as ConformerTransducer._salloc lays it out
        full = torch.zeros((rows + 2 * slack) * width, dtype=dtype, device=dev)
        full[slack * width:(slack + rows) * width] = t.reshape(-1).to(dev)
        return full, full[slack * width:(slack + rows) * width].view(rows, width)

    a1_full, a1 = slacked(SO.to_s2d(x1), 4 * C)
    Wd, bd = W.to(dev), b.to(dev)
    o = nans(dev, rows, C, dtype=dtype)
    if dtype == F32:
        base = slack * 4 * C
        for i in range(9):
            K.gemm(a1_full[base + shift[i] * 4 * C + blk[i] * C:], Wd[i * C:(i + 1) * C], o, rows, C, C, 4 * C, C, C, bias=bd if i == 0 else None, accumulate=i > 0)
    else:
        K.gemm(a1, Wd, o, rows, C, 9 * C, 4 * C, C, C, bias=bd, seg=fwd)
    gemm_close("conv2", o.view(B, T2 + 1, F2 + 1, C)[:, 1:, 1:], r["y"], dtype, 9 * C)
    # the incoming gradient: rows (b, tt, ff) of the S layout's indexing, zero halo
    doh = torch.zeros(B, T2 + 1, F2 + 1, C, dtype=dtype)
    doh[:, 1:, 1:] = dy
    do_full, do = slacked(doh, C)
    gW, gb = torch.zeros(9 * C, C, device=dev), torch.zeros(C, device=dev)
    base = slack * 4 * C
    K.gemm_group([dict(A=a1_full[base + shift[i] * 4 * C + blk[i] * C:], B=do, out=gW[i * C:(i + 1) * C], M=C, N=C, K=rows, lda=4 * C, ldb=C, ldd=C,
                       trans_a=True, accumulate=True, split_k=4, colsum=gb if i == 0 else None) for i in range(9)])
    gemm_close("dW", gW, r["dW"], dtype, B * T2 * F2)
    gemm_close("db", gb, r["db"], dtype, B * T2 * F2)
    da1 = nans(dev, rows, 4 * C, dtype=dtype)
    for b4 in range(4):
        segs, a_off, b_off = dgrad[b4]
        out = da1.view(-1)[b4 * C:]
        if dtype == F32:
            for j, i in enumerate(segs):
                K.gemm(do_full[slack * C - shift[i] * C:], Wd[i * C:(i + 1) * C], out, rows, C, C, C, C, 4 * C, trans_b=True, accumulate=j > 0)
        else:
            K.gemm(do, Wd, out, rows, C, len(segs) * C, C, C, 4 * C, trans_b=True, seg=(a_off, b_off, C // (a_off.numel() // len(segs))))
    gemm_close("da1", SO.from_s2d(da1.cpu().view(B, T2 + 1, F2 + 1, 2, 2, C), T1, F1), r["dx"], dtype, 9 * C)
