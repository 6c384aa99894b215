"""CPU: tfasr_gemm_route / tfasr_gemm_group_route (csrc/gemm_route.h, the one statement of the GEMM dispatch rules) against
gemm_oracle.route(), the independent Python restatement, and against the labels the GPU cases of tests/test_gemm_routes_gpu.py were
written for.  The library is loaded without a GPU, as in tests/test_abi.py; the argument structs point at fake addresses (the route
functions dereference nothing: only null-ness and alignment count).

test_case_table        every case of gemm_oracle.cases(cus) and group_cases() at 64 and 256 compute units: library == oracle == the case's
                       label, and the launch count.  (At 8 and 304 units some labels are not what the rules give - the table sizes M for the
                       routes, not the reverse - so the label check stays at these two counts.)
test_sweep             a deterministic sweep over the fields of gemm_oracle.Case - sizes at every tile and threshold edge, the four
                       layouts, every epilogue combination the oracle models, accumulation with k-splits and column sums, batches, padded
                       and odd row strides, operands and D one element off, f32 - at 64, 256 and 304 units: library == oracle.
test_optional_struct_parts  the same for the parts of the struct route() leaves out, against gemm_oracle.route_full().
test_argument_errors   the statuses tfasr_gemm gives for the calls it refuses."""
import ctypes
import itertools
from dataclasses import replace

import pytest

import gemm_oracle as GO
from tensorflowasr_amd import _lib
from tensorflowasr_amd._lib import ACT_FACTOR, ACT_NONE, ACT_SIGMOID, ACT_SWISH, ACT_TANH, ACT_TANH_OUT

INVALID, UNSUPPORTED = 1, 3
EDGES = [63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 319, 320]
ACTS = [ACT_NONE, ACT_SWISH, ACT_TANH, ACT_SIGMOID]
DACTS = [ACT_NONE, ACT_SWISH, ACT_TANH, ACT_SIGMOID, ACT_TANH_OUT, ACT_FACTOR]
SOME_EPILOGUES = [dict(), dict(bias=True, prez=True, act=ACT_SWISH), dict(bias=True, act=ACT_SWISH, drop_p=0.5), dict(dact=ACT_SWISH),
                  dict(dact=ACT_SWISH, drop_p=0.5), dict(dact=ACT_FACTOR), dict(res=True), dict(res=True, drop_p=0.5), dict(act=ACT_TANH),
                  dict(out_f32=True), dict(dact=ACT_TANH_OUT)]


def _rows_at_thresholds(cus, N):
    """row counts that put the 128-wide tile count just below / above cus and 2 cus, the 64-wide one around 2 cus (the one-tile rule) and the
    count of 256-row tiles (256 and 320 columns) around 2 cus"""
    out = set()
    for rows, width, targets in ((128, 128, (cus, 2 * cus)), (128, 64, (2 * cus,)), (256, 256, (2 * cus,)), (256, 320, (2 * cus,))):
        gx = GO.ceil_div(N, width)
        for t in targets:
            for tiles_y in (t // gx, t // gx + 1):
                if tiles_y >= 1:
                    out.update((rows * tiles_y - 1, rows * tiles_y, rows * tiles_y + 1))
    return sorted(m for m in out if m > 0)


def sweep(cus):
    """the argument sets of test_sweep for a part with `cus` compute units (every one a call tfasr_gemm accepts)"""
    n = itertools.count()
    mk = lambda M, N, K, **kw: GO.mk(f"s{next(n)}", (), M, N, K, **kw)
    # sizes at every tile edge, the four layouts, bf16 and f32
    for (_, ta, tb), M, N, K, dtype in itertools.product(GO.LAYOUTS, EDGES, EDGES, [7, 8] + EDGES, ("bf16", "f32")):
        yield mk(M, N, K, ta=ta, tb=tb, dtype=dtype)
    # row counts at the thresholds that depend on the CU count, a handful of epilogues
    for N, K in itertools.product((64, 65, 128, 129, 192, 256, 257, 320, 384, 640), (64, 120, 128, 264, 512)):
        for M, (_, ta, tb), e in itertools.product(_rows_at_thresholds(cus, N), GO.LAYOUTS, SOME_EPILOGUES[::2]):
            yield mk(M, N, K, ta=ta, tb=tb, **e)
    # every epilogue combination the oracle models, on one shape per route family
    shapes = [(200, 144, 136), (130, 40, 72), (128 * (cus // 2 + 8) - 37, 192, 136), (128 * (GO.ceil_div(2 * cus, 3) + 2) - 37, 192, 136),
              (128 * (GO.ceil_div(cus + 1, 3) + 1) - 37, 384, 320), (256 * 2 * cus + 77, 256, 128), (256 * 2 * cus + 77, 320, 128)]
    for (M, N, K), (_, ta, tb) in itertools.product(shapes, GO.LAYOUTS):
        for act, dact, res, drop, prez, f32out in itertools.product(ACTS, DACTS, (False, True), (0.0, 0.5), (False, True), (False, True)):
            yield mk(M, N, K, ta=ta, tb=tb, act=act, dact=dact, res=res, drop_p=drop, prez=prez, out_f32=f32out, bias=prez)
    # accumulation: k-splits, the fused column sums (transposed-A products only), f32
    for (_, ta, tb), split, M, N, dtype in itertools.product(GO.LAYOUTS, (1, 5, 32), [64, 129, 144, 384] + _rows_at_thresholds(cus, 256)[:6], EDGES + [48, 384],
                                                             ("bf16", "f32")):
        for colsum in ((False, True) if ta and not tb else (False,)):
            yield mk(M, N, 4136, ta=ta, tb=tb, accumulate=True, out_f32=True, split_k=split, colsum=colsum, dtype=dtype)
    # addressing: batches, padded and odd row strides, operands and D one element off
    for (M, N, K), (_, ta, tb), (nb1, nb2), pad, a_off, b_off, d_off, e in itertools.product(
            shapes[:5], GO.LAYOUTS, ((1, 1), (2, 3)), (0, 3, 8), (0, 1), (0, 1), (0, 1), SOME_EPILOGUES[:8]):
        yield mk(M, N, K, ta=ta, tb=tb, nb1=nb1, nb2=nb2, ldd=N + pad, a_off=a_off, b_off=b_off, d_off=d_off, **e)
    # the 256-row kernels' output rules: padded / odd rows, D one element off, both widths, the tanh-out factor
    for N, pad, d_off, tb, dact, K in itertools.product((192, 255, 256, 320, 448, 512, 640), (0, 3, 8), (0, 1), (False, True), (ACT_NONE, ACT_TANH_OUT),
                                                        (120, 127, 128, 136)):
        for M in _rows_at_thresholds(cus, N)[-6:]:
            yield mk(M, N, K, tb=tb, ldd=N + pad, d_off=d_off, dact=dact)
    # f32 with epilogues (the generic kernels' two tile widths)
    for (M, N, K), (_, ta, tb), e in itertools.product([(200, 144, 20), (77, 40, 19), (300, 384, 20), (128 * (2 * cus // 3 + 2), 384, 20)], GO.LAYOUTS, SOME_EPILOGUES):
        yield mk(M, N, K, ta=ta, tb=tb, dtype="f32", **{k: v for k, v in e.items() if k != "out_f32"})


@pytest.mark.parametrize("cus", [64, 256])
def test_case_table(cus):
    table = GO.cases(cus)
    assert len(table) == 157
    for name, c in table.items():
        want = GO.route(c, cus)
        assert GO.library_route(c, cus) == (want, c.launches), f"{name} at {cus} CUs: library {GO.library_route(c, cus)}, oracle {want}, {c.launches} launches"
        assert want == c.label, f"{name} at {cus} CUs: the rules give {want}, the case was written for {c.label}"
    cs = GO.group_cases()
    assert GO.library_route_group(cs, cus) == GO.route_group(cs, cus) == cs[0].label
    # what keeps a group from one launch: a product that is no grouped weight gradient, a single product; 11 products are two chunks
    assert GO.library_route_group(cs[:4] + [replace(cs[4], N=48, ldb=48)], cus) == GO.route_group(cs[:4] + [replace(cs[4], N=48, ldb=48)], cus) == ("one by one",)
    assert GO.library_route_group(cs + cs[:3], cus) == ("group", 128, "E_CSUM")
    n = ctypes.c_int(-1)
    assert _lib.load().tfasr_gemm_group_route(ctypes.byref(GO.gemm_args(cs[0])), 1, cus, ctypes.byref(n)) == 0 and n.value == 1


def test_sweep():
    ran, seen = 0, set()
    for cus in (64, 256, 304):
        for c in sweep(cus):
            want = GO.route(c, cus)
            got, launches = GO.library_route(c, cus)
            assert got == want and launches == (2 if want[0] == "generic+colsum" else 1), f"{c} at {cus} CUs: library {got} ({launches} launches), oracle {want}"
            seen.add(want)
            ran += 1
    print(f"test_sweep: {ran} argument sets, {len(seen)} distinct routes")
    assert ran >= 20000
    assert set(GO.ROUTES) <= seen, f"routes the sweep never reached: {set(GO.ROUTES) - seen}"


def full_sweep(cus):
    """calls with the optional parts of the struct that route() does not model, alone and crossed with each other: K-segments (legal and
    illegal seg_k), row-tile and K-block tables (legal and too long), the row statistics (right and wrong lse_parts, with and without D),
    the gradient epilogue, the BatchNorm sums, accumulation with and without a workspace - refused calls included"""
    n = itertools.count()
    big_m = 256 * 2 * cus + 77
    shapes = [(200, 144, 128), (big_m, 256, 128), (big_m, 320, 192), (big_m, 1000, 128), (big_m - 256 * 8, 256, 128), (300, 64, 128)]
    accs = [dict(), dict(accumulate=True, out_f32=True), dict(accumulate=True, out_f32=True, split_k=4, ws=True)]
    epis = [dict(), dict(res=True), dict(dact=ACT_TANH_OUT), dict(bias=True)]
    for (M, N, K), (_, ta, tb), seg_k, row_tiles, k_tiles, lse, no_D, rgrad, bns, acc, e in itertools.product(
            shapes, GO.LAYOUTS, (0, 64, 96), (0, 1, 1 << 20), (0, 1), (0, 1, 2), (False, True), (False, True), (False, True), accs, epis):
        if (seg_k, row_tiles, k_tiles, lse, no_D, rgrad, bns, acc.get("ws", False)) == (0, 0, 0, 0, False, False, False, False):
            continue  # (test_sweep's ground)
        yield GO.mk(f"f{next(n)}", (), M, N, K, ta=ta, tb=tb, seg_k=seg_k, row_tiles=row_tiles, k_tiles=k_tiles, lse=lse, no_D=no_D, rgrad=rgrad, bns=bns,
                    bns_c=(8 if N % 8 == 0 and M == 300 else 0), **acc, **e)


def test_optional_struct_parts():
    """the routes route() does not model (K-segments with and without a row-tile table, K-block tables, log-softmax statistics, gradient
    epilogue, BatchNorm sums, workspace split-K), crossed with each other: status, kernel and launch count as gemm_oracle.route_full()
    restates them from the dispatcher as it stood before csrc/gemm_route.h"""
    ran, seen = 0, set()
    for cus in (64, 256):
        for c in full_sweep(cus):
            want = GO.route_full(c, cus)
            got = GO.library_route(c, cus)
            assert got == want, f"{c} at {cus} CUs: library {got}, the restated rules {want}"
            seen.add(want[0] if want[0][0] != "fast" else want[0][3])
            ran += 1
    print(f"test_optional_struct_parts: {ran} argument sets; reached {sorted(map(str, seen))}")
    for label in (("seg", 128), ("ktab", 128, "E_CSUM"), "E_LSE", "E_BNS", "E_WS", ("big", 256, "E_LSE", "tr"), ("big", 256, "E_RGRAD", "rows"),
                  ("big-seg", 256, "0", "tr"), ("status", 1), ("status", 3)):
        assert label in seen, f"never reached: {label}"
    # the call of the review: K-segments AND statistics on a product the 256-row kernels do not take is refused, not run without statistics
    assert GO.library_route(GO.mk("seg+lse", (), 200, 144, 128, seg_k=64, lse=1), 256) == (("status", UNSUPPORTED), None)


def test_argument_errors():
    """what tfasr_gemm refuses comes back as its status, from the route function alone"""
    lib = _lib.load()
    base = GO.mk("ok", (), 200, 144, 136)
    wg = replace(base, ta=True, accumulate=True, out_f32=True, lda=200)

    def status(c, **fields):
        a = GO.gemm_args(c)
        for k, v in fields.items():
            setattr(a, k, v)
        info = _lib.GemmRouteInfo()
        st = lib.tfasr_gemm_route(ctypes.byref(a), 256, ctypes.byref(info))
        assert st == info.status
        return st

    assert status(base) == 0 and status(wg) == 0
    for ptr in ("A", "B", "D"):
        assert status(base, **{ptr: None}) == INVALID, ptr
    assert status(replace(base, accumulate=True)) == INVALID                       # accumulate without an f32 output
    assert status(replace(base, split_k=4)) == INVALID                              # k-slices without accumulation
    assert status(replace(wg, split_k=4)) == 0
    for e in (dict(res=True), dict(dact=ACT_SWISH), dict(prez=True), dict(act=ACT_SWISH), dict(drop_p=0.5)):
        assert status(replace(wg, split_k=4, **e)) == INVALID, e                   # k-slices with an epilogue
    for p in (-0.25, 1.0, 1.5):
        assert status(replace(base, drop_p=p)) == INVALID, p
    assert status(replace(base, drop_p=0.99)) == 0
    assert status(replace(wg, colsum=True)) == 0
    assert status(replace(wg, colsum=True, ta=False, lda=136)) == INVALID           # column sums on a product that is not x^T dy
    assert status(replace(wg, colsum=True, tb=True, ldb=136)) == INVALID
    assert status(replace(wg, colsum=True, accumulate=False)) == INVALID
    assert status(replace(wg, colsum=True, nb1=2)) == INVALID
    assert status(wg, k_tiles=GO.BASE, n_k_tiles=1, nb1=-3, nb2=-3) == 0            # batch counts below 1 count as 1, with a K-block table too
    for dim in ("M", "N", "K"):
        assert status(base, **{dim: 0}) == INVALID, dim
    assert status(base, dtype=7) == INVALID
    assert status(base, seg_a_off=GO.BASE, seg_k=64, dtype=_lib.TFASR_F32) == UNSUPPORTED   # K-segments: bf16 kernels only
    assert lib.tfasr_gemm_route(None, 256, ctypes.byref(_lib.GemmRouteInfo())) == INVALID
    assert lib.tfasr_gemm_route(ctypes.byref(GO.gemm_args(base)), 256, None) == INVALID
    assert lib.tfasr_gemm_group_route(None, 2, 256, ctypes.byref(ctypes.c_int(0))) == INVALID
