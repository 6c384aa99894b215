"""Every entry point and launch branch of csrc/norm.hip against the float64 restatements of tests/norm_oracle.py.

Inputs are rounded to the storage type first and the reference is computed from the rounded values.  The backward kernels receive mean /
rstd / fin / bstats that the TEST chose (never the output of the GPU forward), so an error on one side cannot hide one on the other.
Outputs are pre-filled with NaN: an element the kernel does not write fails its comparison.

Exact cases (indexing): inputs from dyadic lattices on which every sum is exact in float32 in any order; the sum-type outputs must equal the
float64 result bit for bit, so one missing or duplicated row fails.
Random cases (numerics), Gaussian mean 0.3, std 1.5, with u = 2^-24:
    elementwise outputs      |gpu - ref| <= 2^-20 M   (+ 2^-8 |ref| for a bf16 output), M = sum of |term| of the element
    sums over rows           |gpu - ref| <= 2^-18 sum |term|  per column
    BatchNorm var            |gpu - ref| <= 2^-16 (mean^2 + var); rstd, scale, shift and the moving statistics by propagation
Every comparison prints max |gpu - ref| / bound before it asserts (pytest -s shows them).

Entry point                          kernels                                                    test
tfasr_layernorm_fwd                  ln_fwd_vec<bf16,32,4>, <bf16,64>, ln_fwd_kernel<bf16|f32>  test_layernorm_forward, ..._without_saved_statistics
tfasr_layernorm_bwd, ..._bwd_drop    ln_bwd_vec<bf16,32|64,2,8>, ln_bwd_kernel<bf16|f32>        test_layernorm_backward, ..._with_dropped_copy
tfasr_layernorm_bwd_part, _part_n,   ln_bwd_vec<...> with `part`, ln_bwd_fold_kernel            test_layernorm_backward_partial_sums_exact
  _part_blocks, _bwd_fold (1 set)
tfasr_layernorm_bwd_fold (1-8 sets)  ln_bwd_fold_kernel / ln_fold_slice                         test_layernorm_fold_exact[*-False]
tfasr_layernorm_bwd_fold_sets        ln_bwd_fold_sets_kernel / ln_fold_slice                    test_layernorm_fold_exact[*-True]
(ldf8, unaligned branch)             ln_fwd_vec, ln_bwd_vec, bn_stats_vec<.,1,.>                test_*_do(es)_not_start_on_16_bytes
tfasr_bn_stats, tfasr_bn_bwd_stats   bn_stats_vec<bf16,0|1,32|64>, bn_stats_kernel<bf16|f32,0|1> test_batchnorm_statistics_exact, ..._random
tfasr_bn_finalize                    bn_finalize_kernel                                         test_batchnorm_finalize, ..._one_pass_variance_at_mean_16_std
tfasr_bn_apply_fwd                   bn_apply_fwd_kernel, bn_apply_fwd_rows_kernel              test_batchnorm_apply_forward
tfasr_bn_finalize_apply_fwd_copies   bn_finalize_apply_fwd_rows_kernel, bn_sum_copies           test_batchnorm_finalize_and_apply_in_one_launch
tfasr_bn_apply_bwd_grads_copies      bn_apply_bwd_kernel (+ tfasr_axpy), bn_apply_bwd_rows_kernel, test_batchnorm_apply_backward, ..._adds_up_copies,
                                     bn_sum_copies                                              ..._parameter_gradients_exact_on_the_flat_route
tfasr_bn_finalize_apply_fwd,         (forward to the two above)                                 test_batchnorm_entry_points_that_forward
  tfasr_bn_apply_bwd_grads, tfasr_bn_apply_bwd
UNSUPPORTED at C = 144 with copies                                                              test_batchnorm_copies_at_a_width_without_row_kernel_are_refused"""
import math

import pytest
import torch

import norm_oracle as NO
from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.kernels import ACT_NONE, ACT_SWISH

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
K_ELEM, K_SUM, K_VAR, K_BF16 = 2.0 ** -20, 2.0 ** -18, 2.0 ** -16, 2.0 ** -8
NAN = float("nan")

# Rows one pass of each grid-stride loop covers, from the launch arithmetic of csrc/norm.hip (past it, a thread makes its second trip).
LN_FWD_VEC32_PASS = 2048 * 4 * 2 * 4  # tfasr_layernorm_fwd, C <= 256: grid <= 2048 blocks x 4 waves x 2 rows per wave x U = 4 in flight
LN_FWD_VEC64_PASS = 2048 * 4 * 1 * 2  # tfasr_layernorm_fwd, 256 < C <= 512: grid <= 2048 x 4 waves x 1 row x U = 2
LN_FWD_GEN_PASS = 2048 * 4            # rows_grid(): <= 256 * 8 blocks x 4 waves, one row per wave
LN_BWD_GEN_PASS = 256 * 4             # tfasr_layernorm_bwd_drop: ln_bwd_kernel's grid <= 256 blocks x 4 waves
RED_VEC32_PASS = 192 * 8 * 2 * 2      # fat_grid(rows, 2): red_grid_cap() = 192 blocks x 8 waves x 2 rows per wave x 2 in flight
RED_VEC64_PASS = 192 * 8 * 1 * 2      # fat_grid(rows, 1)
RED_CAP_RISES = 800000                # fat_grid(): the cap is max(192, rows / 4096): 195 blocks here
BN_STATS_GEN_PASS = 1024 * 4          # tfasr_bn_stats / tfasr_bn_bwd_stats, generic: grid.x <= 1024 blocks x 4 waves
BN_FLAT_PASS = 4096 * 256 * 8         # flat_grid(): <= 256 * 16 blocks x 256 threads x 8 elements
BN_ROWS_GRID = 2048                   # rows_variant_grid(): <= 2048 blocks of rpb = 256 / (C / 8) rows, 2 rows in flight per thread


def _id(v):
    return {BF: "bf16", F32: "f32"}.get(v) if isinstance(v, torch.dtype) else None


def rpb(C):
    return 256 // (C // 8)


# ------------------------------------------------------------------------------------------------------------------------ helpers
def hold(what, got, ref, M, k=K_ELEM, bf16=False, extra=0.0):
    """|got - ref| <= k M (+ 2^-8 |ref| for a bf16 output) (+ extra), everywhere; NaN / inf fail"""
    dt = str(got.dtype).replace("torch.", "")
    got = got.detach().double().cpu().reshape(ref.shape)
    bound = k * M + extra + (K_BF16 * ref.abs() if bf16 else 0.0)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what} ({dt}): max |gpu - ref| / bound = {worst:.3g}")
    bad = ~(err <= bound)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound ({worst:.3g} x at the worst); first at flat index {i}: "
                             f"gpu {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} bound {float(bound.flatten()[i])!r}")


def exact(what, got, ref):
    """got (float32) == ref (float64, representable in float32) bit for bit"""
    got, want = got.detach().cpu().reshape(ref.shape), ref.float()
    assert torch.equal(want.double(), ref), f"{what}: the reference itself is not a float32 value"
    bad = got != want
    if bad.any() or not torch.isfinite(got).all():
        i = int((bad | ~torch.isfinite(got)).flatten().nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} differ; first at {i}: gpu {float(got.flatten()[i])!r} ref {float(want.flatten()[i])!r}")


def gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(int(s) for s in seed)) % (2 ** 31))


def gauss(g, shape, dtype, mean=0.3, std=1.5):
    return (torch.randn(*shape, generator=g) * std + mean).to(dtype)


def lattice(g, shape, step, lim, dtype=F32):
    n = int(round(lim / step))
    return (torch.randint(-n, n + 1, shape, generator=g).float() * step).to(dtype)


def pick(g, shape, values):
    return torch.tensor(values, dtype=F32)[torch.randint(0, len(values), shape, generator=g)]


def fresh(t, dev):
    """a copy on the device that the kernel may add to (never the tensor the expectation is computed from)"""
    return t.to(dev, copy=True)


def nans(dev, *shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def offset_view(t, dev):
    """a copy of the 1-D float32 tensor `t` on the device that starts 4 bytes past a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 8, dtype=F32, device=dev)
    v = buf[1:1 + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def ln_fwd(dev, x, gamma, beta):
    """tfasr_layernorm_fwd into NaN-filled outputs"""
    rows, C = x.shape
    y, mean, rstd = torch.full_like(x, NAN), nans(dev, rows), nans(dev, rows)
    K.check(K._L().tfasr_layernorm_fwd(K._p(x), K._p(gamma), K._p(beta), K._p(y), K._p(mean), K._p(rstd), rows, C, NO.LN_EPS, K._dt(x), K._stream()),
            "layernorm_fwd")
    return y, mean, rstd


# -------------------------------------------------------------------------------------------------------------- LayerNorm forward
LN_FWD_CASES = (
    [(BF, C, rows) for C in (8, 144, 256) for rows in (1, 31, 33)]            # ln_fwd_vec<32, 4>: ragged last group of 4 in-flight rows
    + [(BF, C, LN_FWD_VEC32_PASS + 6) for C in (8, 144)]                      # ... past one pass (one live lane of 32 at C = 8)
    + [(BF, 264, 5)] + [(BF, C, LN_FWD_VEC64_PASS + 3) for C in (264, 512)]   # ln_fwd_vec<64>
    + [(BF, 36, 5), (BF, 36, LN_FWD_GEN_PASS + 3)]                            # ln_fwd_kernel<bf16>: C % 8 != 0
    + [(BF, C, LN_FWD_GEN_PASS + 3) for C in (40, 520, 1024)]                 # (C = 40 is a multiple of 8: the vector kernel takes it), C > 512
    + [(F32, 144, 5)] + [(F32, C, LN_FWD_GEN_PASS + 3) for C in (144, 1024)]  # ln_fwd_kernel<float>
)


@pytest.mark.parametrize("dtype,C,rows", LN_FWD_CASES, ids=_id)
def test_layernorm_forward(dev, dtype, C, rows):
    g = gen(1, C, rows)
    x = gauss(g, (rows, C), dtype)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = NO.layernorm_fwd(x, gamma, beta)
    y, mean, rstd = ln_fwd(dev, x.to(dev), gamma.to(dev), beta.to(dev))
    hold("y", y, ref["y"], ref["M_y"], bf16=dtype == BF)
    hold("mean", mean, ref["mean"], ref["M_mean"])
    hold("rstd", rstd, ref["rstd"], ref["M_rstd"])


@pytest.mark.parametrize("dtype,C", [(BF, 144), (BF, 512), (F32, 40)], ids=_id)
def test_layernorm_forward_without_saved_statistics(dev, dtype, C):
    """save_stats=False passes NULL mean / rstd"""
    g = gen(2, C)
    x = gauss(g, (37, C), dtype)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = NO.layernorm_fwd(x, gamma, beta)
    y, mean, rstd = K.layernorm_fwd(x.to(dev), gamma.to(dev), beta.to(dev), save_stats=False)
    assert mean is None and rstd is None
    hold("y", y, ref["y"], ref["M_y"], bf16=dtype == BF)


# ------------------------------------------------------------------------------------------------------------- LayerNorm backward
LATTICE_WIDE = (2.0, 1.0, (0.5, 1.0, 2.0))   # x in [-2, 2] / 4, mean in [-1, 1] / 4, rstd: terms dy xhat in units of 1/16, at most 96 of them
LATTICE_LONG = (1.0, 0.25, (1.0, 2.0))       # for 800 000 rows: units of 1/8, at most 20


def ln_bwd_inputs(g, rows, C, dtype, kind, lat=LATTICE_WIDE):
    """x, dy, add in `dtype`, mean / rstd float32, gamma.  kind "exact": dyadic lattices on which sum_rows dy xhat and sum_rows dy are exact
    in float32 in any order (asserted here); "random": Gaussian, mean / rstd = the float64 statistics of x rounded to float32."""
    if kind == "exact":
        xlim, mlim, rstds = lat
        x, dy, add = lattice(g, (rows, C), 0.25, xlim, dtype), lattice(g, (rows, C), 0.5, 1.0, dtype), lattice(g, (rows, C), 0.25, 2.0, dtype)
        mean, rstd = lattice(g, (rows,), 0.25, mlim), pick(g, (rows,), rstds)
        unit, top = 0.25 * min(rstds) * 0.5, (xlim + mlim) * max(rstds) * 1.0
        assert (rows + 1) * (top / unit) < 2 ** 24  # (+ 1: the non-zero destination the sums are added to)
    else:
        x, dy, add = gauss(g, (rows, C), dtype), torch.randn(rows, C, generator=g).to(dtype), torch.randn(rows, C, generator=g).to(dtype)
        f = NO.layernorm_fwd(x, torch.ones(C), torch.zeros(C))
        mean, rstd = f["mean"].float(), f["rstd"].float()
    return x, dy, add, mean, rstd, torch.randn(C, generator=g)


def check_sums(kind, ref, dg, db, dg0, db0):
    if kind == "exact":
        exact("dgamma", dg, ref["dgamma"] + dg0)
        exact("dbeta", db, ref["dbeta"] + db0)
    else:
        hold("dgamma", dg, ref["dgamma"] + dg0, ref["M_dgamma"] + abs(dg0), k=K_SUM)
        hold("dbeta", db, ref["dbeta"] + db0, ref["M_dbeta"] + abs(db0), k=K_SUM)


LN_BWD_CASES = (
    [(BF, C, rows) for C in (8, 144, 256) for rows in (1, 33, RED_VEC32_PASS + 7)]  # ln_bwd_vec<32>
    + [(BF, 8, RED_CAP_RISES)]
    + [(BF, C, RED_VEC64_PASS + 5) for C in (264, 512)]                            # ln_bwd_vec<64>
    + [(BF, 36, LN_BWD_GEN_PASS + 3), (BF, 1024, LN_BWD_GEN_PASS + 3), (F32, 144, LN_BWD_GEN_PASS + 3)]  # ln_bwd_kernel
    + [(BF, 40, LN_BWD_GEN_PASS + 3)]                                              # (a multiple of 8: ln_bwd_vec<32>, 5 live lanes)
)


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("dtype,C,rows", LN_BWD_CASES, ids=_id)
def test_layernorm_backward(dev, dtype, C, rows, kind, with_add):
    """tfasr_layernorm_bwd (gamma / beta gradients by atomics, ADDED to their destinations)"""
    g = gen(3, C, rows, with_add)
    x, dy, add, mean, rstd, gamma = ln_bwd_inputs(g, rows, C, dtype, kind, LATTICE_LONG if rows == RED_CAP_RISES else LATTICE_WIDE)
    add = add if with_add else None
    ref = NO.layernorm_bwd(dy, x, gamma, mean, rstd, add)
    dg, db = torch.full((C,), 0.5, device=dev), torch.full((C,), -0.25, device=dev)
    dx = K.layernorm_bwd(dy.to(dev), x.to(dev), gamma.to(dev), mean.to(dev), rstd.to(dev), dg, db, add=None if add is None else add.to(dev),
                         dx=torch.full_like(x, NAN).to(dev))
    hold("dx", dx, ref["dx"], ref["M_dx"], bf16=dtype == BF)
    check_sums(kind, ref, dg, db, 0.5, -0.25)


@pytest.mark.parametrize("dtype,C", [(BF, 144), (BF, 36), (F32, 144)], ids=_id)
def test_layernorm_backward_with_dropped_copy(dev, dtype, C):
    """the second output is K.dropout of the ROUNDED dx, bit for bit, and dx itself is the oracle's"""
    g = gen(4, C)
    rows = 33
    x, dy, add, mean, rstd, gamma = ln_bwd_inputs(g, rows, C, dtype, "random")
    ref = NO.layernorm_bwd(dy, x, gamma, mean, rstd, add)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dropped = torch.full_like(x, NAN).to(dev)
    dx = K.layernorm_bwd(dy.to(dev), x.to(dev), gamma.to(dev), mean.to(dev), rstd.to(dev), dg, db, add=add.to(dev), dx=torch.full_like(x, NAN).to(dev),
                         dropped=dropped, drop_p=0.1, drop_seed=12345)
    hold("dx", dx, ref["dx"], ref["M_dx"], bf16=dtype == BF)
    check_sums("random", ref, dg, db, 0.0, 0.0)
    assert torch.equal(dropped, K.dropout(dx, 0.1, 12345))
    assert 0 < int((dropped == 0).sum()) < dropped.numel() // 2
    if K.layernorm_bwd_part_blocks(rows, C, dtype) > 0:  # the partial-sum route writes the same two outputs
        part, dropped2 = nans(dev, 7, 2 * C), torch.full_like(x, NAN).to(dev)
        dx2 = K.layernorm_bwd_part_n(dy.to(dev), x.to(dev), gamma.to(dev), mean.to(dev), rstd.to(dev), part, nblk=7, add=add.to(dev),
                                     dx=torch.full_like(x, NAN).to(dev), dropped=dropped2, drop_p=0.1, drop_seed=12345)
        assert torch.equal(dx2, dx) and torch.equal(dropped2, dropped)


# ------------------------------------------------------------------------------------------------- LayerNorm partial sums and folds
def rows_per_block(C):
    return 8 * (2 if C <= 256 else 1)  # ln_bwd_vec_kernel<., LPR, 2, 8>: 8 waves x 64 / LPR rows (the first of the 2 rows in flight)


@pytest.mark.parametrize("C,rows,nblk", [(40, 777, None), (144, 777, None), (256, RED_VEC32_PASS + 7, None), (512, RED_VEC64_PASS + 5, None),
                                         (256, 777, 1), (256, 777, 3), (256, 777, 5), (256, 777, 256), (40, 333, 5), (40, 333, 256), (512, 100, 256)])
def test_layernorm_backward_partial_sums_exact(dev, C, rows, nblk):
    """tfasr_layernorm_bwd_part (nblk None: its own slot count) / tfasr_layernorm_bwd_part_n: the slots add up to the oracle's dgamma / dbeta
    bit for bit, slots whose block has no rows hold exactly zero, and tfasr_layernorm_bwd_fold adds the column sums to its destinations."""
    g = gen(5, C, rows, nblk or 0)
    x, dy, add, mean, rstd, gamma = ln_bwd_inputs(g, rows, C, BF, "exact")
    ref = NO.layernorm_bwd(dy, x, gamma, mean, rstd, add)
    nb = nblk or K.layernorm_bwd_part_blocks(rows, C, BF)
    assert nb >= 1
    part = nans(dev, nb, 2 * C)
    dx = K.layernorm_bwd_part_n(dy.to(dev), x.to(dev), gamma.to(dev), mean.to(dev), rstd.to(dev), part, nblk=nblk, add=add.to(dev),
                                dx=torch.full_like(x, NAN).to(dev))
    hold("dx", dx, ref["dx"], ref["M_dx"], bf16=True)
    p = part.cpu()
    assert torch.isfinite(p).all()
    exact("sum of the slots", p.double().sum(0).float(), torch.cat([ref["dgamma"], ref["dbeta"]]))
    first_empty = -(-rows // rows_per_block(C))
    if nblk is not None and first_empty < nb:
        assert bool((p[first_empty:] == 0).all()), "a slot without rows is not zero"
    dg, db = torch.full((C,), 0.5, device=dev), torch.full((C,), -0.25, device=dev)
    K.layernorm_bwd_fold_parts(part, nb, C, [dg], [db])
    check_sums("exact", ref, dg, db, 0.5, -0.25)


@pytest.mark.parametrize("nsets,separate", [(1, False), (3, False), (8, False), (1, True), (3, True), (20, True)])
@pytest.mark.parametrize("nblk", [1, 3, 5, 22, 256])  # thread groups with empty ranges (1, 3), scalar tail only (5), unrolled + tail (22), unrolled only
@pytest.mark.parametrize("C", [40, 256])              # 2C = 80 is no multiple of the 64-column slice
def test_layernorm_fold_exact(dev, C, nblk, nsets, separate):
    """tfasr_layernorm_bwd_fold (sets back to back) and tfasr_layernorm_bwd_fold_sets (sets in separate buffers): destination += column sums
    of the set's nblk slots, bit for bit on lattice values; a NULL dgamma / dbeta entry is skipped."""
    g = gen(6, C, nblk, nsets, separate)
    part = lattice(g, (nsets, nblk, 2 * C), 1.0 / 16, 4.0)
    assert (nblk + 1) * 64 < 2 ** 24
    dg0, db0 = lattice(g, (nsets, C), 0.25, 2.0), lattice(g, (nsets, C), 0.25, 2.0)
    dgs, dbs = [fresh(t, dev) for t in dg0], [fresh(t, dev) for t in db0]
    if nsets >= 3:
        dgs[1], dbs[2] = None, None
    if separate:
        parts = [part[i].contiguous().to(dev) for i in range(nsets)]
        K.layernorm_bwd_fold_sets(parts, nblk, C, dgs, dbs)
    else:
        K.layernorm_bwd_fold_parts(part.to(dev), nblk, C, dgs, dbs)
    want = part.double().sum(1)
    for i in range(nsets):
        if dgs[i] is not None:
            exact(f"dgamma[{i}]", dgs[i], dg0[i].double() + want[i, :C])
        if dbs[i] is not None:
            exact(f"dbeta[{i}]", dbs[i], db0[i].double() + want[i, C:])


# ---------------------------------------------------------------------------------------------------------- unaligned parameters
@pytest.mark.parametrize("C", [144, 264])
def test_layernorm_with_parameters_that_do_not_start_on_16_bytes(dev, C):
    """gamma / beta as views offset by one float: the dword branch of ldf8 in ln_fwd_vec and ln_bwd_vec"""
    g = gen(7, C)
    rows = 33
    x = gauss(g, (rows, C), BF)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    gv, bv = offset_view(gamma, dev), offset_view(beta, dev)
    ref = NO.layernorm_fwd(x, gamma, beta)
    y, mean, rstd = ln_fwd(dev, x.to(dev), gv, bv)
    hold("y", y, ref["y"], ref["M_y"], bf16=True)
    hold("mean", mean, ref["mean"], ref["M_mean"])
    hold("rstd", rstd, ref["rstd"], ref["M_rstd"])
    x, dy, add, mean, rstd, _ = ln_bwd_inputs(g, rows, C, BF, "exact")
    refb = NO.layernorm_bwd(dy, x, gamma, mean, rstd, add)
    dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    dx = K.layernorm_bwd(dy.to(dev), x.to(dev), gv, mean.to(dev), rstd.to(dev), dg, db, add=add.to(dev), dx=torch.full_like(x, NAN).to(dev))
    hold("dx", dx, refb["dx"], refb["M_dx"], bf16=True)
    check_sums("exact", refb, dg, db, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------- BatchNorm statistics
def lattice_fin(g, C):
    """fin with mean in multiples of 1/4 and rstd a power of two (scale / shift arbitrary: act = none does not read them)"""
    return torch.cat([lattice(g, (C,), 0.25, 1.0), pick(g, (C,), (0.5, 1.0, 2.0)), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1])


def random_fin(x, g, count=None):
    """the float64 finalize of x's own moments, rounded to float32: gamma in [0.5, 1.5), small beta"""
    C = x.shape[-1]
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    return NO.bn_finalize(NO.bn_moments(x)["stats"], count or x.shape[0], gamma, beta)["fin"].float()


BN_STATS_CASES = (
    [(BF, C, rows) for C in (8, 144, 256) for rows in (1, RED_VEC32_PASS - 1, RED_VEC32_PASS + 7)]     # bn_stats_vec<32>
    + [(BF, C, rows) for C in (264, 640, 1280) for rows in (1, RED_VEC64_PASS - 1, RED_VEC64_PASS + 5)]  # bn_stats_vec<64>: 1, 2, 3 slabs (last partial)
    + [(dt, C, rows) for dt, C in ((F32, 144), (F32, 1280), (BF, 36)) for rows in (1, BN_STATS_GEN_PASS - 1, BN_STATS_GEN_PASS + 3)]  # bn_stats_kernel
)


@pytest.mark.parametrize("dtype,C,rows", BN_STATS_CASES, ids=_id)
def test_batchnorm_statistics_exact(dev, dtype, C, rows):
    """tfasr_bn_stats (sum x, sum x^2) and tfasr_bn_bwd_stats with act = none (sum dy, sum dy xhat), ADDED to their destination: bit for bit"""
    g = gen(8, C, rows)
    x, dy, fin = lattice(g, (rows, C), 0.25, 2.0, dtype), lattice(g, (rows, C), 0.5, 1.0, dtype), lattice_fin(g, C)
    assert (rows + 1) * 96 < 2 ** 24  # x^2 <= 64 units of 1/16; dy xhat <= (2 + 1) * 2 * 1 = 96 units of 1/16
    stats = torch.full((2 * C,), 0.25, device=dev)
    K.bn_stats(x.to(dev), stats)
    exact("stats", stats, NO.bn_moments(x)["stats"] + 0.25)
    bstats = torch.full((2 * C,), -0.5, device=dev)
    K.bn_bwd_stats(x.to(dev), dy.to(dev), fin.to(dev), bstats, ACT_NONE)
    exact("bstats", bstats, NO.bn_bwd_sums(x, dy, fin)["bstats"] - 0.5)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_SWISH])
@pytest.mark.parametrize("dtype,C,rows", [(BF, C, RED_VEC32_PASS + 7) for C in (8, 144, 256)] + [(BF, C, RED_VEC64_PASS + 5) for C in (264, 640, 1280)]
                         + [(dt, C, BN_STATS_GEN_PASS + 3) for dt, C in ((F32, 144), (F32, 1280), (BF, 36))], ids=_id)
def test_batchnorm_statistics_random(dev, dtype, C, rows, act):
    g = gen(9, C, rows)
    x, dy = gauss(g, (rows, C), dtype), torch.randn(rows, C, generator=g).to(dtype)
    fin = random_fin(x, g)
    stats, bstats = torch.zeros(2 * C, device=dev), torch.zeros(2 * C, device=dev)
    K.bn_stats(x.to(dev), stats)
    K.bn_bwd_stats(x.to(dev), dy.to(dev), fin.to(dev), bstats, act)
    m, s = NO.bn_moments(x), NO.bn_bwd_sums(x, dy, fin, act == ACT_SWISH)
    hold("stats", stats, m["stats"], m["M_stats"], k=K_SUM)
    hold("bstats", bstats, s["bstats"], s["M_bstats"], k=K_SUM)


@pytest.mark.parametrize("C", [144, 640])
def test_batchnorm_backward_sums_with_fin_that_does_not_start_on_16_bytes(dev, C):
    """fin as a view offset by one float: the dword branch of ldf8 in bn_stats_vec MODE 1"""
    g = gen(10, C)
    rows = 77
    x, dy, fin = lattice(g, (rows, C), 0.25, 2.0, BF), lattice(g, (rows, C), 0.5, 1.0, BF), lattice_fin(g, C)
    bstats = torch.zeros(2 * C, device=dev)
    K.bn_bwd_stats(x.to(dev), dy.to(dev), offset_view(fin, dev), bstats, ACT_NONE)
    exact("bstats", bstats, NO.bn_bwd_sums(x, dy, fin)["bstats"])
    x, dy = gauss(g, (rows, C), BF), torch.randn(rows, C, generator=g).to(BF)
    fin = random_fin(x, g)
    bstats.zero_()
    K.bn_bwd_stats(x.to(dev), dy.to(dev), offset_view(fin, dev), bstats, ACT_SWISH)
    s = NO.bn_bwd_sums(x, dy, fin, True)
    hold("bstats swish", bstats, s["bstats"], s["M_bstats"], k=K_SUM)


# ------------------------------------------------------------------------------------------------------------ BatchNorm finalize
def split_copies(g, total, copies):
    """float32 [copies, n] of uneven shares of `total`; returns them and their float64 sum (what the kernel is given)"""
    w = torch.rand(copies, 1, generator=g).double() + 0.05
    w[0] *= 5
    c = (total.double()[None, :] * (w / w.sum())).float()
    return c, c.double().sum(0)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("C", [144, 256, 1280])
def test_batchnorm_finalize(dev, C, training):
    """tfasr_bn_finalize: fin and the momentum update (training), the moving statistics untouched (inference)"""
    g = gen(11, C, training)
    rows = 500
    x = gauss(g, (rows, C), F32)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    mm0, mv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    m = NO.bn_moments(x)
    stats = m["stats"].float()
    ref = NO.bn_finalize(stats, rows, gamma, beta, mm0, mv0, training=training)
    bnd = NO.bn_finalize_bounds(ref, m["M_stats"], rows, gamma, beta, mm0, mv0, training=training)
    fin, mm, mv = nans(dev, 4 * C), fresh(mm0, dev), fresh(mv0, dev)
    K.bn_finalize(stats.to(dev) if training else None, rows, gamma.to(dev), beta.to(dev), fin, mm, mv, training=training)
    hold("fin", fin, ref["fin"], bnd["fin"], k=1.0)
    if training:
        hold("moving_mean", mm, ref["moving_mean"], bnd["moving_mean"], k=1.0)
        hold("moving_var", mv, ref["moving_var"], bnd["moving_var"], k=1.0)
    else:
        assert torch.equal(mm.cpu(), mm0) and torch.equal(mv.cpu(), mv0)


@pytest.mark.parametrize("dtype,C", [(F32, 144), (BF, 256)], ids=_id)
def test_batchnorm_one_pass_variance_at_mean_16_std(dev, dtype, C):
    """|mean| / std = 16: S1 / n - (S0 / n)^2 cancels 8 bits.  Held to |var - ref| <= 2^-16 (mean^2 + var) only (a float32 one-pass restatement in
    numpy gave 8e-6 relative at this ratio, 5e-4 at 64): it documents the cancellation and asks for no other algorithm."""
    g = gen(12, C)
    rows = BN_STATS_GEN_PASS + 3
    x = gauss(g, (rows, C), dtype, mean=16.0, std=1.0)
    ones, zeros = torch.ones(C), torch.zeros(C)
    ref = NO.bn_finalize(NO.bn_moments(x)["stats"], rows, ones, zeros)
    stats, fin, mm, mv = torch.zeros(2 * C, device=dev), nans(dev, 4 * C), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    K.bn_stats(x.to(dev), stats)
    K.bn_finalize(stats, rows, ones.to(dev), zeros.to(dev), fin, mm, mv)
    var = mv.double().cpu() / (1 - float(torch.tensor(NO.BN_MOMENTUM, dtype=F32)))  # moving_var was 0: it now holds var (1 - momentum)
    hold("var", var, ref["var"], ref["mean"] ** 2 + ref["var"], k=K_VAR)


# ------------------------------------------------------------------------------------------------- BatchNorm apply, forward and backward
BN_APPLY_CASES = (
    [(dt, 144, rows, act) for dt in (F32, BF) for rows in (1, 37) for act in (ACT_NONE, ACT_SWISH)]                   # flat kernels
    + [(F32, 1280, 6600, ACT_NONE), (BF, 1280, 6600, ACT_SWISH)]                                                      # ... past one grid
    + [(dt, C, rows, act) for dt in (F32, BF) for C in (64, 256) for rows in (1, rpb(C) + 1) for act in (ACT_NONE, ACT_SWISH)]  # row kernels; rpb + 1: the `two == false` tail
    + [(dt, 2048, rows, act) for dt in (F32, BF) for rows in (1, 2) for act in (ACT_NONE, ACT_SWISH)]
    + [(F32, 2048, 2 * BN_ROWS_GRID * rpb(2048) + 3, ACT_SWISH), (BF, 2048, 2 * BN_ROWS_GRID * rpb(2048) + 3, ACT_NONE)]  # ... past one pass
)
assert 1280 * 6600 > BN_FLAT_PASS and 256 % (1280 // 8) != 0  # (C = 1280 has no row kernel)


def bn_inputs(g, rows, C, dtype):
    """x, dy, and a fin whose statistics are those of a larger batch around x (count rows + 50), so one row is no degenerate case"""
    x, dy = gauss(g, (rows, C), dtype), torch.randn(rows, C, generator=g).to(dtype)
    fin = random_fin(gauss(g, (rows + 50, C), dtype), g)
    return x, dy, fin


@pytest.mark.parametrize("dtype,C,rows,act", BN_APPLY_CASES, ids=_id)
def test_batchnorm_apply_forward(dev, dtype, C, rows, act):
    """tfasr_bn_apply_fwd: y = act(x scale + shift).  Swish runs on the fast exponential and the hardware reciprocal; measured against the
    oracle over these float32 cases it stays at 0.19 of the bound (3 ulp of M), so it is held to the same 2^-20 M as act = none (0.06)."""
    g = gen(13, C, rows, act)
    x, _, fin = bn_inputs(g, rows, C, dtype)
    ref = NO.bn_apply(x, fin, act == ACT_SWISH)
    y = K.bn_apply_fwd(x.to(dev), fin.to(dev), act, y=torch.full_like(x, NAN).to(dev))
    hold("y", y, ref["y"], ref["M_y"], bf16=dtype == BF)


@pytest.mark.parametrize("dtype,C,rows,act,grads", [c + ("both",) for c in BN_APPLY_CASES]
                         + [c + (gr,) for c in BN_APPLY_CASES if c[2] == 37 or c[1:3] == (256, rpb(256) + 1) for gr in ("no_dgamma", "no_dbeta")], ids=_id)
def test_batchnorm_apply_backward(dev, dtype, C, rows, act, grads):
    """tfasr_bn_apply_bwd_grads_copies, copies = 1: dx from fin and bstats the test chose, dgamma / dbeta += grad_scale * the statistics (NULL
    entries skipped).  swish' on the fast exponential, float32, measured against the oracle over these cases: 0.51 of the bound (8 ulp of M,
    where M counts swish'(z) = s + s z (1 - s) by its two terms: it passes through zero at z = -1.278); act = none 0.19.  Both are held to
    2^-20 M."""
    g = gen(14, C, rows, act)
    x, dy, fin = bn_inputs(g, rows, C, dtype)
    count = rows + 50
    bstats = (NO.bn_bwd_sums(x, dy, fin, act == ACT_SWISH)["bstats"] * 1.25).float()
    ref = NO.bn_bwd_apply(x, dy, fin, bstats, count, act == ACT_SWISH)
    dg0, db0 = lattice(g, (C,), 0.25, 2.0), lattice(g, (C,), 0.25, 2.0)
    dg, db = (None if grads == "no_dgamma" else fresh(dg0, dev)), (None if grads == "no_dbeta" else fresh(db0, dev))
    dx = K.bn_apply_bwd(x.to(dev), dy.to(dev), fin.to(dev), bstats.to(dev), count, act, dx=torch.full_like(x, NAN).to(dev), dgamma=dg, dbeta=db, grad_scale=0.5)
    hold("dx", dx, ref["dx"], ref["M_dx"], bf16=dtype == BF)
    b = bstats.double()
    if dg is not None:
        hold("dgamma", dg, dg0.double() + 0.5 * b[C:], dg0.abs().double() + 0.5 * b[C:].abs())
    if db is not None:
        hold("dbeta", db, db0.double() + 0.5 * b[:C], db0.abs().double() + 0.5 * b[:C].abs())


@pytest.mark.parametrize("copies", [1, 2, 8])
@pytest.mark.parametrize("dtype,C,rows,act", [(F32, 64, 33, ACT_SWISH), (BF, 256, 9, ACT_NONE), (BF, 256, 300, ACT_SWISH), (F32, 2048, 2, ACT_NONE),
                                              (BF, 2048, 2 * BN_ROWS_GRID + 3, ACT_SWISH)], ids=_id)
def test_batchnorm_apply_backward_adds_up_copies(dev, dtype, C, rows, act, copies):
    """bstats spread unevenly over [copies][2C]: the row kernel adds them up (bn_sum_copies); dgamma / dbeta exact on lattice statistics"""
    g = gen(15, C, rows, copies)
    x, dy, fin = bn_inputs(g, rows, C, dtype)
    count = rows + 50
    total = NO.bn_bwd_sums(x, dy, fin, act == ACT_SWISH)["bstats"]
    cps, tot = split_copies(g, total, copies)
    ref = NO.bn_bwd_apply(x, dy, fin, tot, count, act == ACT_SWISH)
    dx = K.bn_apply_bwd(x.to(dev), dy.to(dev), fin.to(dev), cps.to(dev), count, act, dx=torch.full_like(x, NAN).to(dev), copies=copies)
    # (the float32 sum of the copies adds <= copies * u of sum |copy| = |S| to the S0 / S1 terms of M)
    hold("dx", dx, ref["dx"], ref["M_dx"], k=K_ELEM + copies * NO.U, bf16=dtype == BF)
    lat = lattice(g, (copies, 2 * C), 1.0 / 16, 4.0)
    dg0, db0 = lattice(g, (C,), 0.25, 2.0), lattice(g, (C,), 0.25, 2.0)
    dg, db = fresh(dg0, dev), fresh(db0, dev)
    K.bn_apply_bwd(x.to(dev), dy.to(dev), fin.to(dev), lat.to(dev), count, act, dgamma=dg, dbeta=db, grad_scale=0.25, copies=copies)
    s = lat.double().sum(0)
    exact("dgamma", dg, dg0.double() + 0.25 * s[C:])
    exact("dbeta", db, db0.double() + 0.25 * s[:C])


@pytest.mark.parametrize("dtype,C", [(F32, 256), (BF, 144)], ids=_id)
def test_batchnorm_entry_points_that_forward(dev, dtype, C):
    """tfasr_bn_finalize_apply_fwd (= ..._copies with one copy; C = 144: UNSUPPORTED), tfasr_bn_apply_bwd_grads (= ..._grads_copies with one
    copy) and tfasr_bn_apply_bwd (= ..._grads without parameter gradients), called through the C ABI"""
    g = gen(19, C)
    rows, count = 37, 87
    L, p, dt, st = K._L(), K._p, K._dt, K._stream
    x, dy, fin = bn_inputs(g, rows, C, dtype)
    bstats = NO.bn_bwd_sums(x, dy, fin, True)["bstats"].float()
    xd, dyd, find, bsd = x.to(dev), dy.to(dev), fin.to(dev), bstats.to(dev)  # (named: a pointer must not outlive its tensor)
    ref = NO.bn_bwd_apply(x, dy, fin, bstats, count, True)
    dg0, db0 = lattice(g, (C,), 0.25, 2.0), lattice(g, (C,), 0.25, 2.0)
    dg, db, dx = fresh(dg0, dev), fresh(db0, dev), torch.full_like(xd, NAN)
    K.check(L.tfasr_bn_apply_bwd_grads(p(xd), p(dyd), p(find), p(bsd), float(count), p(dx), rows, C, ACT_SWISH, p(dg), p(db), 2.0, dt(xd),
                                       st()), "bn_apply_bwd_grads")
    hold("dx", dx, ref["dx"], ref["M_dx"], bf16=dtype == BF)
    b = bstats.double()
    hold("dgamma", dg, dg0.double() + 2 * b[C:], dg0.abs().double() + 2 * b[C:].abs())
    hold("dbeta", db, db0.double() + 2 * b[:C], db0.abs().double() + 2 * b[:C].abs())
    dx = torch.full_like(xd, NAN)
    K.check(L.tfasr_bn_apply_bwd(p(xd), p(dyd), p(find), p(bsd), float(count), p(dx), rows, C, ACT_SWISH, dt(xd), st()), "bn_apply_bwd")
    hold("dx", dx, ref["dx"], ref["M_dx"], bf16=dtype == BF)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    mm0, mv0 = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    m = NO.bn_moments(gauss(g, (count, C), dtype))
    stats = m["stats"].float()
    f = NO.bn_finalize(stats, count, gamma, beta, mm0, mv0)
    bnd = NO.bn_finalize_bounds(f, m["M_stats"], count, gamma, beta, mm0, mv0)
    finw, mm, mv, y = nans(dev, 4 * C), fresh(mm0, dev), fresh(mv0, dev), torch.full_like(xd, NAN)
    sd, gd, bd = stats.to(dev), gamma.to(dev), beta.to(dev)
    status = L.tfasr_bn_finalize_apply_fwd(p(xd), p(sd), float(count), p(gd), p(bd), p(finw), p(mm), p(mv), NO.BN_MOMENTUM,
                                           NO.BN_EPS, p(y), rows, C, ACT_SWISH, 1, dt(xd), st())
    torch.cuda.synchronize()
    if C == 144:
        assert status == _lib.STATUS_UNSUPPORTED and bool(torch.isnan(y).all()) and bool(torch.isnan(finw).all()) and torch.equal(mm.cpu(), mm0)
        return
    assert status == 0
    hold("fin", finw, f["fin"], bnd["fin"], k=1.0)
    hold("moving_mean", mm, f["moving_mean"], bnd["moving_mean"], k=1.0)
    hold("moving_var", mv, f["moving_var"], bnd["moving_var"], k=1.0)
    a = NO.bn_apply(x, f["fin"], True)
    hold("y", y, a["y"], a["M_y"], bf16=dtype == BF, extra=1.1 * (x.double().abs() * bnd["scale"] + bnd["shift"]))


@pytest.mark.parametrize("dtype", [F32, BF], ids=_id)
def test_batchnorm_apply_backward_parameter_gradients_exact_on_the_flat_route(dev, dtype):
    """C = 144 (no row kernel): dgamma / dbeta through tfasr_axpy"""
    g = gen(16)
    C, rows = 144, 37
    x, dy, fin = bn_inputs(g, rows, C, dtype)
    lat = lattice(g, (2 * C,), 1.0 / 16, 4.0)
    dg0, db0 = lattice(g, (C,), 0.25, 2.0), lattice(g, (C,), 0.25, 2.0)
    dg, db = fresh(dg0, dev), fresh(db0, dev)
    K.bn_apply_bwd(x.to(dev), dy.to(dev), fin.to(dev), lat.to(dev), rows, ACT_NONE, dgamma=dg, dbeta=db, grad_scale=0.25)
    exact("dgamma", dg, dg0.double() + 0.25 * lat[C:].double())
    exact("dbeta", db, db0.double() + 0.25 * lat[:C].double())


def test_batchnorm_copies_at_a_width_without_row_kernel_are_refused(dev):
    """C = 144 with copies > 1: UNSUPPORTED, and nothing is written"""
    g = gen(17)
    C, rows = 144, 37
    x, dy, fin = bn_inputs(g, rows, C, BF)
    cps = torch.ones(2, 2 * C, device=dev)
    dx, dg, db = torch.full_like(x, NAN).to(dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    with pytest.raises(_lib.TfasrError):
        K.bn_apply_bwd(x.to(dev), dy.to(dev), fin.to(dev), cps, rows, ACT_NONE, dx=dx, dgamma=dg, dbeta=db, copies=2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and float(dg.abs().sum()) == 0 and float(db.abs().sum()) == 0
    y, f = torch.full_like(x, NAN).to(dev), nans(dev, 4 * C)
    for copies in (1, 2):  # the fused forward has no flat route at all
        assert K.bn_finalize_apply_fwd(x.to(dev), cps, rows, torch.ones(C, device=dev), torch.zeros(C, device=dev), f, dg, db, y=y, copies=copies) is None
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(f).all())


ROW_KERNEL_CASES = [(F32, 64, 33, ACT_SWISH), (BF, 256, 9, ACT_NONE), (BF, 256, 300, ACT_SWISH), (F32, 2048, 2, ACT_NONE),
                    (BF, 2048, 2 * BN_ROWS_GRID + 3, ACT_SWISH), (F32, 256, 1, ACT_NONE)]


@pytest.mark.parametrize("dtype,C,rows,act,copies,training", [c + (n, True) for c in ROW_KERNEL_CASES for n in (1, 2, 8)]
                         + [c + (1, False) for c in ROW_KERNEL_CASES], ids=_id)  # (inference reads no statistics: one case per shape)
def test_batchnorm_finalize_and_apply_in_one_launch(dev, dtype, C, rows, act, copies, training):
    """tfasr_bn_finalize_apply_fwd_copies: statistics spread unevenly over the copies, compared with the float64 finalize of their sum; fin and
    the moving statistics carry bn_finalize's values after ONE update (2048 workgroups derive them, one writes); y through the GPU's own
    scale / shift, so its bound adds their propagated ones: |x| d scale + d shift."""
    g = gen(18, C, rows, copies, training)
    x = gauss(g, (rows, C), dtype)
    count = rows + 50
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    mm0, mv0 = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    m = NO.bn_moments(gauss(g, (count, C), dtype))
    cps, tot = split_copies(g, m["stats"], copies)
    ref = NO.bn_finalize(tot, count, gamma, beta, mm0, mv0, training=training)
    bnd = NO.bn_finalize_bounds(ref, m["M_stats"] * (1 + copies * NO.U / K_SUM), count, gamma, beta, mm0, mv0, training=training)
    fin, mm, mv = nans(dev, 4 * C), fresh(mm0, dev), fresh(mv0, dev)
    y = K.bn_finalize_apply_fwd(x.to(dev), cps.to(dev) if training else None, count, gamma.to(dev), beta.to(dev), fin, mm, mv, act=act,
                                y=torch.full_like(x, NAN).to(dev), training=training, copies=copies)
    assert y is not None
    hold("fin", fin, ref["fin"], bnd["fin"], k=1.0)
    if training:
        hold("moving_mean", mm, ref["moving_mean"], bnd["moving_mean"], k=1.0)
        hold("moving_var", mv, ref["moving_var"], bnd["moving_var"], k=1.0)
    else:
        assert torch.equal(mm.cpu(), mm0) and torch.equal(mv.cpu(), mv0)
    a = NO.bn_apply(x, ref["fin"], act == ACT_SWISH)
    # |swish'| <= 1.1
    hold("y", y, a["y"], a["M_y"], bf16=dtype == BF, extra=1.1 * (x.double().abs() * bnd["scale"] + bnd["shift"]))
