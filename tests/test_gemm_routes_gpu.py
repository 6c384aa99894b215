"""tfasr_gemm and tfasr_gemm_group on every dispatch route and epilogue against the float64 restatement of tests/gemm_oracle.py.

Every case first asserts that gemm_oracle.route(), the Python restatement of the dispatcher, AND the library's own route (tfasr_gemm_route)
give the label the case was written for at the LIVE compute-unit count, then the launch count of the call (1; 2 for the column-sum
fallback), then the results.  Inputs are rounded to the storage type first; operand buffers hold NaN wherever the product must not read
(row padding, the k tail of a padded row, the element in front of an operand that starts off 16 bytes); D and prez are pre-filled with NaN,
guard columns (ldd > N), a guard row and the gaps between batches included, and everything outside the M x N views must come back bit for
bit.  dact_z, res, the start values and the masks are the test's own: nothing the GPU produced reaches the reference, except the dropout
mask, which is tfasr_dropout's over a flat buffer of ones (the GEMM epilogues must draw the same mask at doff + row * ldd + col).

exact kind   operands integers in [-3, 3], alpha / beta powers of two, bias / res / start values multiples of 1/4, FACTOR / TANH_OUT inputs
             multiples of 1/8, p in {0.5, 0.75}: every partial sum is below 2^24 in any order, slice split or atomic order, so f32 outputs
             must EQUAL the float64 reference and bf16 outputs reference.float().to(bfloat16); one lost, doubled or misplaced row, column,
             k index or slab fails.  prez is held to equality in every exact case.  Where the chain has a non-linear function (swish,
             tanh, sigmoid, their derivatives), its argument is still exact and the output is held to the suite's element bound for
             these functions (rtol 1e-5, atol 1e-6 on the function value, test_pointwise_gpu._elem_bound) carried through the rest of the
             chain, plus one f32 rounding per further multiply / add and 2^-8 |ref| for a bf16 output.
random kind  Gaussian operands, alpha = 2^-ceil(log2 sqrt K), p = 0.1:  |gpu - ref| <= (K + 2) 2^-23 S  (S = sum_k |alpha a b| + |bias|;
             a start value counts as one more term), carried through the chain the same way (act: times sup |act'|); + 2^-8 |ref| for bf16.
dropout      a dropped element is exactly 0 (exactly res with a residual); the kept share lies within 4 standard deviations of 1 - p.
No bound had to be set from a measurement: on an f32 output the device's fast exponential stays at 0.016 (swish) and 0.043 (swish') of the
element bound (the *-gen_f32_swish and *-gen_dswish_f32 cases, MI355X); bf16 outputs sit at the bf16 rounding itself.  Every comparison prints max |gpu - ref| / bound before it asserts (pytest -s); the worst ratio per
case goes to profiles/gemm_routes_parity.json (0 = equal).

entry point                kernel instantiation                                              test (ids of test_route)
tfasr_gemm, bf16 fast      gemm_fast_kernel<TA,TB,64,0>, all four layouts                     p64-*-nn|nt|tn|tt, p64-k77-lda80
  launch_epi<TA,TB,64,EPI>   <0,0,64,E_RES>, <0,0,64,E_RES|E_DROP>                            p64-*-res, -res_drop, p64c-batched-res_drop
  persistent kernel          <0,0,64,E_ACT>, <0,0,64,E_ACT|E_DROP>                            p64c-act, p64c-act_drop (+ -ldd+8, -ldd+3)
                             <0,1,64,E_DACT>, <0,1,64,E_DACT|E_DROP>, <0,1,64,E_MUL>          p64c-dact, p64c-dact_drop, p64c-mul
                             <*,*,64,E_GEN>                                                   p64-*-gen_*, p64-small-*-is-gen
                             <1,0,64,0> atomics, <1,0,64,E_CSUM>                              wg64-split1|5|8, wg64-split*-colsum
  one tile per workgroup   gemm_fast_one_kernel<TA,TB,0>                                      o64-plain-nn, o64-plain-tn
                             <0,0,E_RES>, <0,0,E_RES|E_DROP>, <0,0,E_ACT>, <0,0,E_ACT|E_DROP>  o64-res, -res_drop, -act, -act_drop
                             <0,1,E_DACT>, <0,1,E_DACT|E_DROP>, <0,1,E_MUL>, <*,*,E_GEN>      o64-dact, -dact_drop, -mul, o64-gen_*
  launch_epi<TA,TB,128,EPI>  gemm_fast_kernel<TA,TB,128,0>, all four layouts                  p128-plain-*, p128-k333-lda344, p128x-plain-*
                             <0,0,128,E_RES|E_RES|E_DROP|E_ACT|E_ACT|E_DROP>                  p128-res, -res_drop, -act, -act_drop, p128x-res_drop
                             <0,1,128,E_DACT|E_DACT|E_DROP|E_MUL>, <*,*,128,E_GEN>            p128-dact, -dact_drop, -mul, p128-gen_*, p128x-dact_drop
                             <1,0,128,0> atomics, <1,0,128,E_CSUM>                            wg128-split32, wg128-split32-colsum
  output addressing          ldd = N + 8, N + 3 (element-wise stores, per-element dropout     p64c|o64|p128-ldd+8|+3-res_drop|act_drop|dact_drop,
                             hash, plain-load fallback of the dact_z prefetch), odd doff,     p64c|o64|p128-batched-*,
                             D / res / dact_z / prez starting off 16 bytes                    p64c|o64|p128-d-off-2-bytes-*
tfasr_gemm, 256-row tiles  gemm_big_kernel<0|1,256,0,false,true> (tr), <0,256,0,false> (rows)  big256-nn, big256-nt, big256-nn-ldd259
                           gemm_big_kernel<1,320,0,false>                                     big320-nt
                           gemm_big_kernel<1,256,E_DACT,false,true>, <1,320,E_DACT,false>     big256-nt-tanh_out, big320-nt-tanh_out
tfasr_gemm, generic        gemm_kernel<bf16,TA,TB> per refusal rule of tfasr_gemm_fast_try     gbf-*
                           gemm_kernel<float,TA,TB,64>, gemm_kernel<float,TA,TB,128>          gf32-200x144x20-*, gf32-77x40x19-*, gf32-wide-n384
                           64- and 128-wide f32 tiles give the same bits                      test_f32_tile_widths_give_the_same_bits
                           tfasr_colsum + gemm_kernel<bf16|float,1,0> (two launches)          wg-n48-colsum, wg-f32-colsum
tfasr_gemm_group           wgrad_group_kernel<E_CSUM,2,128> (one launch)                      test_grouped_weight_gradients"""
import json
import math
import os

import pytest
import torch

import gemm_oracle as GO
from tensorflowasr_amd import kernels as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
SEED = 20240607
PARAMS = [(name, kind) for name, c in GO.cases(256).items() for kind in c.kinds]  # (the names do not depend on the CU count)
_PARITY = {}
_TABLES = {}


@pytest.fixture(scope="module", autouse=True)
def parity_profile():
    yield
    want = {f"{n}/{k}" for n, k in PARAMS} | {f"group/{k}" for k in ("exact", "random")} | {"f32-tile-widths"}
    if want <= set(_PARITY):  # (a partial run leaves the file alone)
        try:
            with open(os.path.join(ROOT, "profiles", "gemm_routes_parity.json"), "w") as f:
                json.dump({"what": "tests/test_gemm_routes_gpu.py: worst max |gpu - ref| / bound per case over D, prez and colsum (0: the "
                                   "comparison was for equality and held); bounds as in that module's docstring",
                           "cases": {k: _PARITY[k] for k in sorted(_PARITY)}}, f, indent=1)
                f.write("\n")
        except OSError:
            pass


def _cus(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def _case(dev, name):
    cus = _cus(dev)
    if cus not in _TABLES:
        _TABLES[cus] = GO.cases(cus)
    c = _TABLES[cus][name]
    assert GO.route(c, cus) == c.label, f"{name}: on {cus} CUs the dispatcher takes {GO.route(c, cus)}, the case was written for {c.label}"
    assert GO.library_route(c, 0) == (c.label, c.launches), f"{name}: the library takes {GO.library_route(c, 0)}, the case was written for {c.label}"
    return c


def _note(key, ratio):
    _PARITY[key] = max(_PARITY.get(key, 0.0), float(ratio))


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def _equal(key, what, got, want64, dtype):
    """got == the float64 reference rounded once to the output type; NaN fails"""
    want = want64.float()
    assert torch.equal(want.double(), want64), f"{what}: the reference itself is not a float32 value"
    want = want.to(dtype).float()
    got = got.float()
    bad = ~(got == want)
    print(f"{key} {what}: {int(bad.sum())} of {bad.numel()} differ (equality)")
    _note(key, 0.0 if not bad.any() else math.inf)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{key} {what}: {int(bad.sum())} of {bad.numel()} differ; first at {i}: gpu {float(got[i])!r} ref {float(want[i])!r}")


def _hold(key, what, got, ref, bound):
    got = got.double()
    bound = torch.broadcast_to(bound, ref.shape)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, math.inf))
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{key} {what}: max |gpu - ref| / bound = {worst:.3g}")
    _note(key, worst)
    bad = ~(err <= bound)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{key} {what}: {int(bad.sum())} of {bad.numel()} outside the bound ({worst:.3g} x at the worst); first at {i}: "
                             f"gpu {float(got[i])!r} ref {float(ref[i])!r} bound {float(bound[i])!r}")


def _untouched(key, what, c, got, fill):
    """everything outside the [nb1, nb2, M, N] view of the flat buffer still holds the bits it was filled with"""
    outside = torch.ones(got.numel(), dtype=torch.bool)
    GO.d_view(c, outside).fill_(False)
    assert int((~outside).sum()) == c.nb * c.M * c.N
    same = _bits(got)[outside] == _bits(fill)[outside]
    assert bool(same.all()), f"{key} {what}: {int((~same).sum())} elements outside the M x N views were written"


def _setup(dev, c, x):
    """device buffers of one call and its keyword arguments for kernels.gemm / gemm_group"""
    st, dt = (F32 if c.f32 else BF), (F32 if c.d_f32 else BF)
    b = dict(A=x["A"].to(st).to(dev), B=x["B"].to(st).to(dev))
    b["fill_D"] = (x["start"] if c.accumulate else torch.full((c.d_len(),), NAN)).to(dt)
    b["D"] = b["fill_D"].clone().to(dev)
    for k in ("res", "dact_z"):
        b[k] = x[k].to(st).to(dev) if k in x else None
    b["bias"] = x["bias"].to(dev) if c.bias else None
    b["prez"] = torch.full((c.d_len(),), NAN, dtype=st, device=dev) if c.prez else None
    b["colsum"] = torch.cat([x["colsum_start"], torch.full((8,), NAN)]).to(dev) if c.colsum else None
    b["keep"] = None
    if c.drop_p > 0:
        mask = (K.dropout(torch.ones(c.d_len() - c.d_off, device=dev), c.drop_p, SEED) != 0).cpu()  # index 0 = the element D points at
        b["keep"] = torch.cat([torch.zeros(c.d_off, dtype=torch.bool), mask])
    off = lambda t: None if t is None else t[c.d_off:]
    kw = dict(A=b["A"][c.a_off:], B=b["B"][c.b_off:], out=b["D"][c.d_off:], M=c.M, N=c.N, K=c.K, lda=c.lda, ldb=c.ldb, ldd=c.ldd, trans_a=c.ta, trans_b=c.tb,
              bias=b["bias"], res=off(b["res"]), dact_z=off(b["dact_z"]), prez=off(b["prez"]), alpha=c.alpha, beta=c.beta, act=c.act, dact=c.dact, nb1=c.nb1,
              nb2=c.nb2, sA=c.sA, sB=c.sB, sD=c.sD, accumulate=c.accumulate, split_k=c.split_k, drop_p=c.drop_p, drop_seed=SEED, colsum=b["colsum"])
    return b, kw


def _judge(key, c, x, b, kind):
    exact = kind == "exact"
    dt = F32 if c.d_f32 else BF
    r = GO.reference(c, x["A"], x["B"], x.get("bias"), x.get("dact_z"), b["keep"], c.drop_p, x.get("res"), x.get("start"), x.get("colsum_start"),
                     want_S=False, sum_exact=exact)
    got = b["D"].cpu()
    _untouched(key, "D", c, got, b["fill_D"])
    gv = GO.d_view(c, got)
    if exact and not c.nonlinear:
        _equal(key, "D", gv, r["D"], dt)
    else:
        _hold(key, "D", gv, r["D"], GO.bound(r["E"], r["D"], dt == BF))
    if c.prez:
        st = F32 if c.f32 else BF
        gp = b["prez"].cpu()
        _untouched(key, "prez", c, gp, torch.full((c.d_len(),), NAN, dtype=st))
        if exact:
            _equal(key, "prez", GO.d_view(c, gp), r["prez"], st)
        else:
            _hold(key, "prez", GO.d_view(c, gp), r["prez"], GO.bound(r["E_prez"], r["prez"], st == BF))
    if c.colsum:
        gc = b["colsum"].cpu()
        assert bool(torch.isnan(gc[c.N:]).all()), f"{key}: colsum written past N"
        if exact:
            _equal(key, "colsum", gc[:c.N], r["colsum"], F32)
        else:
            _hold(key, "colsum", gc[:c.N], r["colsum"], r["E_colsum"])
    if c.drop_p > 0:
        kp = GO.d_view(c, b["keep"])
        want0 = GO.d_view(c, x["res"]).to(dt).float() if c.res else torch.zeros(())
        dropped = torch.where(kp, torch.zeros(()), (gv.float() - want0).abs())
        assert float(dropped.max()) == 0, f"{key}: a dropped element is not exactly {'res' if c.res else '0'}"
        n, q = kp.numel(), 1.0 - c.drop_p
        share = float(kp.double().mean())
        print(f"{key} dropout: kept share {share:.5f} of {n}, expected {q} +- {math.sqrt(q * (1 - q) / n):.2g}")
        assert abs(share - q) <= 4 * math.sqrt(q * (1 - q) / n), f"{key}: kept share {share} of {n} elements at p = {c.drop_p}"


@pytest.mark.parametrize("name,kind", PARAMS, ids=[f"{n}-{k}" for n, k in PARAMS])
def test_route(dev, name, kind):
    c0 = _case(dev, name)
    c, x = GO.make_inputs(c0, kind)
    assert GO.route(c, _cus(dev)) == c0.label
    if kind == "exact":
        assert GO.largest_partial_sum(c, x) < 2 ** 24
    b, kw = _setup(dev, c, x)
    n0 = K.launch_count()
    K.gemm(**kw)
    n1 = K.launch_count()
    torch.cuda.synchronize()
    assert n1 - n0 == c.launches, f"{name}: {n1 - n0} launches, {c.launches} expected for {c.label}"
    _judge(f"{name}/{kind}", c, x, b, kind)


@pytest.mark.parametrize("kind", ["exact", "random"])
def test_grouped_weight_gradients(dev, kind):
    """tfasr_gemm_group: eight weight gradients (with and without the fused bias gradient, K = 1000 / 993 / 150, ragged edges, start values
    not zero) in ONE launch, each held to its own float64 reference"""
    cs = GO.group_cases()
    assert GO.route_group(cs, _cus(dev)) == ("group", 128, "E_CSUM")
    assert GO.library_route_group(cs, 0) == ("group", 128, "E_CSUM")
    runs = []
    for c0 in cs:
        c, x = GO.make_inputs(c0, kind)
        runs.append((c, x) + _setup(dev, c, x))
    n0 = K.launch_count()
    K.gemm_group([kw for _, _, _, kw in runs])
    n1 = K.launch_count()
    torch.cuda.synchronize()
    assert n1 - n0 == 1, f"{n1 - n0} launches for the group"
    for c, x, b, _ in runs:
        _judge(f"group/{kind}", c, x, b, kind)


def test_f32_tile_widths_give_the_same_bits(dev):
    """launch<float> takes 128 x 64 tiles below 2 CUs tiles and 128 x 128 ones from there on - 'same slabs, same k order per element:
    bitwise the same results' (csrc/gemm.hip).  The first 300 rows of the wide product, computed alone (narrow tiles), on Gaussian data."""
    wide, narrow = _case(dev, "gf32-wide-n384"), _case(dev, "gf32-wide-n384-first-300-rows")
    assert wide.label[2] == 128 and narrow.label[2] == 64 and (wide.N, wide.K, wide.lda) == (narrow.N, narrow.K, narrow.lda)
    c, x = GO.make_inputs(wide, "random")
    b, kw = _setup(dev, c, x)
    K.gemm(**kw)
    alone = torch.full((narrow.M * narrow.N,), NAN, device=dev)
    n0 = K.launch_count()
    K.gemm(**{**kw, "out": alone, "M": narrow.M})
    assert K.launch_count() - n0 == 1
    torch.cuda.synchronize()
    both = b["D"][:narrow.M * narrow.N].cpu()
    assert bool(torch.isfinite(both).all())
    same = _bits(both) == _bits(alone.cpu())
    print(f"f32 tile widths: {int((~same).sum())} of {same.numel()} elements differ")
    _note("f32-tile-widths", 0.0 if bool(same.all()) else math.inf)
    assert bool(same.all())
