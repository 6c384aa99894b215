"""tests/gemm_oracle.py on the CPU: reference() against a triple loop over the flat buffers, route() against the label every row of the
case table was written for (at 256 compute units, the MI355X), and the lattice property the bitwise comparisons of
tests/test_gemm_routes_gpu.py rest on."""
import collections
import math

import pytest
import torch

import gemm_oracle as GO
from tensorflowasr_amd import _lib
from tensorflowasr_amd._lib import ACT_FACTOR, ACT_NONE, ACT_SIGMOID, ACT_SWISH, ACT_TANH, ACT_TANH_OUT

CUS = 256
TABLE = GO.cases(CUS)


def _sig(x):
    return 1.0 / (1.0 + math.exp(-x))


ACT = {ACT_NONE: lambda v: v, ACT_SWISH: lambda v: v * _sig(v), ACT_TANH: math.tanh, ACT_SIGMOID: _sig}
DACT = {ACT_SWISH: lambda z: _sig(z) * (1 + z * (1 - _sig(z))), ACT_TANH: lambda z: 1 - math.tanh(z) ** 2, ACT_SIGMOID: lambda z: _sig(z) * (1 - _sig(z)),
        ACT_TANH_OUT: lambda z: 1 - z * z, ACT_FACTOR: lambda z: z}


def _loops(c, x, keep, p):
    """the call element by element, with the index arithmetic of gemm_kernel (csrc/gemm.hip) written out"""
    A, B = x["A"].double().tolist(), x["B"].double().tolist()
    D = torch.full((c.nb1, c.nb2, c.M, c.N), GO.NAN, dtype=torch.float64)
    Z, S = D.clone(), D.clone()
    cs = x["colsum_start"].double().clone() if c.colsum else None
    for b1 in range(c.nb1):
        for b2 in range(c.nb2):
            oa, ob, od = c.a_off + b1 * c.sA[0] + b2 * c.sA[1], c.b_off + b1 * c.sB[0] + b2 * c.sB[1], b1 * c.sD[0] + b2 * c.sD[1]
            for i in range(c.M):
                for j in range(c.N):
                    acc = s = 0.0
                    for k in range(c.K):
                        a = A[oa + (k * c.lda + i if c.ta else i * c.lda + k)]
                        b = B[ob + (j * c.ldb + k if c.tb else k * c.ldb + j)]
                        acc += a * b
                        s += abs(c.alpha * a * b)
                    idx = od + i * c.ldd + j
                    v = c.alpha * acc + (float(x["bias"][j]) if c.bias else 0.0)
                    s += abs(float(x["bias"][j])) if c.bias else 0.0
                    Z[b1, b2, i, j] = v
                    v = ACT[c.act](v)
                    if c.dact != ACT_NONE:
                        v *= DACT[c.dact](float(x["dact_z"][idx]))
                    if keep is not None:
                        v = v / (1.0 - p) if bool(keep[idx]) else 0.0
                    if c.res:
                        v = float(x["res"][idx]) + c.beta * v
                    if c.accumulate:
                        v += float(x["start"][idx])
                        s += abs(float(x["start"][idx]))
                    D[b1, b2, i, j], S[b1, b2, i, j] = v, s
    if c.colsum:
        for j in range(c.N):
            for k in range(c.K):
                cs[j] += c.alpha * B[c.b_off + k * c.ldb + j]
    return D, Z, S, cs


TINY = [
    GO.mk("tiny-nn-chain", (), 5, 7, 9, bias=True, prez=True, act=ACT_SWISH, dact=ACT_TANH, drop_p=0.5, res=True, ldd=11, a_off=1),
    GO.mk("tiny-nt-batched", (), 4, 6, 11, tb=True, nb1=2, nb2=3, bias=True, dact=ACT_TANH_OUT, drop_p=0.75, res=True, ldd=9, b_off=3),
    GO.mk("tiny-tn-accumulate-colsum", (), 6, 5, 13, ta=True, accumulate=True, out_f32=True, colsum=True, split_k=3),
    GO.mk("tiny-tt-f32", (), 3, 4, 5, ta=True, tb=True, dtype="f32", act=ACT_SIGMOID, dact=ACT_FACTOR, lda=5, ldb=7),
    GO.mk("tiny-nn-dswish", (), 3, 9, 8, dact=ACT_SWISH, act=ACT_TANH, bias=True),
    GO.mk("tiny-nt-dsigmoid", (), 2, 3, 4, tb=True, dact=ACT_SIGMOID),
]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("case", TINY, ids=[c.name for c in TINY])
def test_reference_agrees_with_a_triple_loop(case, kind):
    c, x = GO.make_inputs(case, kind)
    keep = None
    if c.drop_p > 0:
        keep = torch.rand(c.d_len(), generator=torch.Generator().manual_seed(5)) >= c.drop_p
    r = GO.reference(c, x["A"], x["B"], x.get("bias"), x.get("dact_z"), keep, c.drop_p, x.get("res"), x.get("start"), x.get("colsum_start"))
    D, Z, S, cs = _loops(c, x, keep, float(torch.tensor(c.drop_p, dtype=torch.float32)))  # (the C ABI passes p as a float)
    for name, got, want in (("D", r["D"], D), ("prez", r["prez"], Z), ("S", r["S"], S)):
        assert torch.isfinite(want).all()
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12, msg=lambda m: f"{c.name} {name}: {m}")
    if c.colsum:
        torch.testing.assert_close(r["colsum"], cs, rtol=1e-12, atol=1e-12)
    # the bound: nothing but roundings - zero for a linear chain on exact sums, and never below the sum bound on random ones
    e = GO.reference(c, x["A"], x["B"], x.get("bias"), x.get("dact_z"), keep, c.drop_p, x.get("res"), x.get("start"), x.get("colsum_start"), sum_exact=True)
    assert torch.equal(e["D"], r["D"]) and "S" not in e
    assert float(torch.as_tensor(e["E_prez"]).abs().max()) == 0
    if not (c.res or c.dact != ACT_NONE or c.drop_p > 0 or c.act != ACT_NONE):
        n = c.K + (3 if c.accumulate else 2)
        assert torch.equal(torch.broadcast_to(r["E"], S.shape), n * GO.U23 * r["S"])


def test_activation_constants_are_the_librarys():
    assert (ACT_NONE, ACT_SWISH, ACT_TANH, ACT_SIGMOID, ACT_TANH_OUT, ACT_FACTOR) == (0, 1, 2, 3, 4, 5)
    assert (GO.ACT_SWISH, GO.ACT_FACTOR) == (_lib.ACT_SWISH, _lib.ACT_FACTOR)


@pytest.mark.parametrize("name", list(TABLE))
def test_route_gives_the_label_the_case_was_written_for(name):
    c = TABLE[name]
    assert GO.route(c, CUS) == c.label
    assert c.launches == (2 if c.label[0] == "generic+colsum" else 1)
    assert c.ldd >= c.N and c.lda >= c.a_shape[1] and c.ldb >= c.b_shape[1]
    assert set(c.kinds) <= {"exact", "random"} and "exact" in c.kinds
    if c.drop_p > 0:
        assert c.drop_p in (0.5, 0.75)  # 1 / (1 - p) = 2 or 4: exact


def test_every_route_has_an_exact_and_a_random_case():
    seen = collections.Counter((c.label, k) for c in TABLE.values() for k in c.kinds)
    missing = [(r, k) for r in GO.ROUTES for k in ("exact", "random") if not seen[(r, k)]]
    assert not missing, missing
    assert {c.label for c in TABLE.values()} <= set(GO.ROUTES), "a label the route list does not name"
    assert GO.route_group(GO.group_cases(), CUS) == ("group", 128, "E_CSUM")
    assert GO.route_group(GO.group_cases()[:1], CUS) == ("one by one",)
    assert GO.route_group([GO.mk("f32", (), 144, 200, 1000, ta=True, accumulate=True, out_f32=True, dtype="f32")] * 2, CUS) == ("one by one",)


def test_the_sizes_follow_the_cu_count():
    """on a part with another CU count the builders give the same routes (where the rule itself does not name a fixed shape)"""
    for cus in (64, 104, 304):
        for name, c in GO.cases(cus).items():
            if name.startswith(("p64c", "o64", "p128", "big", "gf32-wide")):
                assert GO.route(c, cus) == c.label, (cus, name, GO.route(c, cus))


def test_refusal_rules_of_the_fast_path():
    base = dict(M=200, N=144, K=136)
    assert GO._fast_refusal(GO.mk("ok", (), **base)) is None
    assert GO._fast_refusal(GO.mk("k", (), 200, 144, 7))
    assert GO._fast_refusal(GO.mk("a", (), a_off=1, **base)) and GO._fast_refusal(GO.mk("b", (), b_off=4, **base))
    assert GO._fast_refusal(GO.mk("a8", (), a_off=8, **base)) is None
    assert GO._fast_refusal(GO.mk("lda", (), lda=139, **base)) and GO._fast_refusal(GO.mk("ldb", (), ldb=148, **base))
    assert GO._fast_refusal(GO.mk("n36", (), 130, 36, 72, ldb=36)) and GO._fast_refusal(GO.mk("m36", (), 36, 144, 72, ta=True, lda=36))
    assert GO._fast_refusal(GO.mk("f32", (), dtype="f32", **base))


@pytest.mark.parametrize("name", [n for n, c in TABLE.items() if c.M * c.N <= 200 * 400] + ["wg128-split32-colsum", "big320-nt-tanh_out"])
def test_exact_inputs_lie_on_the_lattice(name):
    """largest sum_k |a b| below 2^24 (here: K max|a| max|b|, which bounds every partial sum in any order), operands integers in [-3, 3],
    everything else dyadic and exactly representable in the storage type; NaN wherever the product must not read"""
    c, x = GO.make_inputs(TABLE[name], "exact")
    assert GO.largest_partial_sum(c, x) <= 9 * c.K < 2 ** 24 and c.K <= 5000
    st = torch.float32 if c.f32 else torch.bfloat16
    for key, step in (("A", 1.0), ("B", 1.0), ("bias", 0.25), ("res", 0.25), ("start", 0.25), ("colsum_start", 0.25), ("dact_z", 0.125)):
        if key in x:
            v = x[key][~torch.isnan(x[key])]
            assert torch.equal(v / step, torch.round(v / step)) and (key in ("bias", "start", "colsum_start") or torch.equal(v.to(st).float(), v))
    assert math.log2(c.alpha) == round(math.log2(c.alpha)) and math.log2(c.beta) == round(math.log2(c.beta))
    a = GO.a_view(c, x["A"])
    assert float(a.abs().max()) <= 3 and int(torch.isnan(x["A"]).sum()) == x["A"].numel() - a.numel()
    assert int(torch.isnan(x["B"]).sum()) == x["B"].numel() - c.nb * c.K * c.N


def test_every_case_of_the_table_is_on_the_lattice_by_construction():
    """the cases too large to draw here: the bound K * 3 * 3 of their partial sums"""
    for c in list(TABLE.values()) + GO.group_cases():
        assert 9 * c.K < 2 ** 24 and c.K <= 5000, c.name
