"""tests/subsampling_oracle.py checked without a GPU: against oracle/conformer_ref.py, against torch.nn.functional.conv2d and torch autograd,
through its own adjoint / round-trip identities, and - the detection condition - that the bounds test_conv2d_gpu.py applies to the sparse
gradient cases are tight enough to see ONE lost or doubled position."""
import pytest
import torch
import torch.nn.functional as F

import subsampling_oracle as SO
from oracle import conformer_ref as R

F64 = torch.float64
SHAPES = [(3, 37, 80, 64), (2, 50, 17, 256), (3, 2801, 9, 16)]  # B, T0, F0, C


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=F64) * scale


@pytest.mark.parametrize("B,T0,F0,C", [(2, 21, 80, 32), (3, 6, 7, 8), (1, 1, 1, 8), (2, 2, 5, 16)])
def test_conv1_against_the_reference_convolution_and_conv2d(B, T0, F0, C):
    g = SO.gen(1, B, T0, F0, C)
    x, w, b = rnd(g, B, T0, F0), rnd(g, 3, 3, 1, C, scale=0.3), rnd(g, C, scale=0.1)
    z, M = SO.conv1(x, w, b)
    T1, F1, _, _ = SO.dims(T0, F0)
    assert z.shape == (B, T1, F1, C)
    torch.testing.assert_close(z, R.conv2d_causal_s2(x[..., None], w, b), rtol=0, atol=1e-13)
    direct = F.conv2d(F.pad(x[:, None], (2, 0, 2, 0)), w.permute(3, 2, 0, 1), b, stride=2).permute(0, 2, 3, 1)
    torch.testing.assert_close(z, direct, rtol=0, atol=1e-13)
    assert (M >= z.abs() - 1e-13).all()
    torch.testing.assert_close(SO.conv1(x, w, None)[0], z - b, rtol=0, atol=1e-13)
    # the weight gradient against autograd
    dy = rnd(g, B, T1, F1, C)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    R.conv2d_causal_s2(x[..., None], wr, br).backward(dy)
    r = SO.conv1_weight_grad(x, dy)
    torch.testing.assert_close(r["dw"], wr.grad.reshape(9, C), rtol=0, atol=1e-12 * float(r["M_dw"].max()))
    torch.testing.assert_close(r["db"], br.grad, rtol=0, atol=1e-12 * float(r["M_db"].max()))


@pytest.mark.parametrize("B,T1,F1,C", [(3, 13, 40, 16), (2, 12, 39, 8), (1, 1, 1, 8)])
def test_conv2_against_the_reference_convolution_and_the_patch_matrix(B, T1, F1, C):
    g = SO.gen(2, B, T1, F1, C)
    x1, W, b = rnd(g, B, T1, F1, C), rnd(g, 9 * C, C, scale=0.1), rnd(g, C, scale=0.1)
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    dy = rnd(g, B, T2, F2, C)
    r = SO.conv2(x1, W, b, dy)
    x1r, Wr = x1.clone().requires_grad_(True), W.clone().requires_grad_(True)
    ref = R.conv2d_causal_s2(x1r, Wr.reshape(3, 3, C, C), b)
    ref.backward(dy)
    torch.testing.assert_close(r["y"], ref.detach(), rtol=0, atol=1e-12)
    torch.testing.assert_close(SO.conv2(x1, W, b), ref.detach(), rtol=0, atol=1e-12)
    torch.testing.assert_close(r["dx"], x1r.grad, rtol=0, atol=1e-12)
    torch.testing.assert_close(r["dW"], Wr.grad, rtol=0, atol=1e-11)
    # ... and as patch matrix x weight matrix: im2col, and col2im for the data gradient
    col = SO.im2col(x1)
    torch.testing.assert_close((col @ W + b).reshape(B, T2, F2, C), r["y"], rtol=0, atol=1e-12)
    torch.testing.assert_close(SO.col2im(dy.reshape(-1, C) @ W.T, B, T1, F1, C), r["dx"], rtol=0, atol=1e-12)
    torch.testing.assert_close(col.T @ dy.reshape(-1, C), r["dW"], rtol=0, atol=1e-11)
    torch.testing.assert_close(r["db"], dy.sum((0, 1, 2)), rtol=0, atol=1e-12)


@pytest.mark.parametrize("B,T1,F1,C", [(2, 5, 7, 8), (3, 6, 4, 8), (1, 1, 1, 8), (2, 1, 6, 16)])
def test_col2im_is_the_adjoint_of_im2col(B, T1, F1, C):
    g = SO.gen(3, B, T1, F1, C)
    x = rnd(g, B, T1, F1, C)
    col = SO.im2col(x)
    c = rnd(g, *col.shape)
    lhs, rhs = float((col * c).sum()), float((x * SO.col2im(c, B, T1, F1, C)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((col * c).abs().sum())


@pytest.mark.parametrize("B,T0,F0", [(2, 9, 7), (1, 1, 1), (3, 6, 8)])
def test_patches_and_gram(B, T0, F0):
    g = SO.gen(4, B, T0, F0)
    x = rnd(g, B, T0, F0)
    p = SO.patches(x)
    T1, F1, _, _ = SO.dims(T0, F0)
    unf = F.unfold(F.pad(x[:, None], (2, 0, 2, 0)), 3, stride=2).view(B, 9, T1, F1)
    assert torch.equal(p, unf)
    gm = SO.gram(x)
    flat = p.permute(1, 0, 2, 3).reshape(9, -1)
    torch.testing.assert_close(gm[:81].reshape(9, 9), flat @ flat.T, rtol=0, atol=1e-11)
    torch.testing.assert_close(gm[81:90], flat.sum(1), rtol=0, atol=1e-11)
    assert float(gm[90]) == B * T1 * F1
    # the statistics through the Gram matrix are the statistics of z
    w, b = rnd(g, 3, 3, 1, 8, scale=0.3), rnd(g, 8, scale=0.1)
    z, M = SO.conv1(x, w, b)
    a, c = SO.stats(z, M), SO.stats_from_gram(gm, w, b)
    torch.testing.assert_close(a["stats"], c["stats"], rtol=0, atol=1e-11 * float(c["M_stats"].max()))
    assert (a["M_stats"] >= a["stats"].abs() - 1e-9).all() and (c["M_stats"] >= c["stats"].abs() - 1e-9).all()


@pytest.mark.parametrize("B,T1,F1", [(2, 5, 7), (3, 6, 4), (1, 1, 1), (2, 5, 4), (2, 6, 7)])
def test_s_layout_round_trip(B, T1, F1):
    C = 8
    dense = torch.arange(1, B * T1 * F1 * C + 1, dtype=F64).reshape(B, T1, F1, C)
    s = SO.to_s2d(dense, fill=float("nan"))
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    assert s.shape == (B, T2 + 1, F2 + 1, 2, 2, C)
    m = SO.valid_mask(B, T1, F1)
    assert int(m.sum()) == B * T1 * F1
    assert torch.equal(torch.isnan(s[..., 0]), ~m)          # exactly the slots that hold no element kept the fill
    assert not m[:, 0].any() and not m[:, :, 0].any()       # the halo
    assert torch.equal(SO.from_s2d(s, T1, F1), dense)
    # the address the kernels use: ((((b (T2+1) + t/2 + 1) (F2+1) + f/2 + 1) 4 + (t%2) 2 + f%2) C
    flat = s.reshape(-1)
    for b, t, f in [(0, 0, 0), (B - 1, T1 - 1, F1 - 1), (B - 1, T1 // 2, F1 // 2)]:
        off = ((((b * (T2 + 1) + t // 2 + 1) * (F2 + 1) + f // 2 + 1) * 4) + (t % 2) * 2 + f % 2) * C
        assert torch.equal(flat[off:off + C], dense[b, t, f])


def autograd_bn0(x, w, b, gamma, beta, dy):
    """conv -> BatchNormalization on the batch statistics -> swish, differentiated by torch"""
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    gr, ber = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    z = R.conv2d_causal_s2(x[..., None], wr, br)
    mean, var = z.mean((0, 1, 2)), z.var((0, 1, 2), unbiased=False)
    yn = (z - mean) * (var + float(torch.tensor(1e-3, dtype=torch.float32))) ** -0.5 * gr + ber
    (yn * torch.sigmoid(yn)).backward(dy)
    return z.detach(), wr.grad.reshape(9, -1), br.grad, gr.grad, ber.grad


@pytest.mark.parametrize("B,T0,F0,C", SHAPES)
def test_bn0_backward_against_autograd(B, T0, F0, C):
    """with fin in float64 the closed form IS the gradient: 1e-12 of max |dw| leaves room for the cancellation in float64 (the terms are
    30 - 150 x max |dw|, N up to 21 000 positions) and nothing else; the float32 rounding of fin alone would move dw by 1e-7"""
    g = SO.gen(5, B, T0, F0, C)
    x = SO.logmel_like(g, (B, T0, F0), F64)
    w, b = rnd(g, 3, 3, 1, C, scale=0.3), rnd(g, C, scale=0.1)
    gamma, beta = 1.0 + rnd(g, C, scale=0.2), rnd(g, C, scale=0.1)
    T1, F1, _, _ = SO.dims(T0, F0)
    dy = rnd(g, B, T1, F1, C, scale=0.5)
    z, dw, db, dgamma, dbeta = autograd_bn0(x, w, b, gamma, beta, dy)
    N = B * T1 * F1
    fin = SO.finalize(SO.stats(z)["stats"], N, gamma, beta)
    r = SO.bn0_backward(x, w, b, fin, dy, N, N)
    top = float(dw.abs().max())
    for name in ("dw", "dw_onepass"):
        err = float((r[name] - dw).abs().max())
        print(f"{name}: {err / top:.3g} of max |dw|")
        assert err <= 1e-12 * top
    torch.testing.assert_close(r["bstats"][:C], dbeta, rtol=0, atol=1e-11 * float(r["M_bstats"][:C].max()))
    torch.testing.assert_close(r["bstats"][C:], dgamma, rtol=0, atol=1e-11 * float(r["M_bstats"][C:].max()))
    # the bias in front of a BatchNorm has no gradient: both routes say "zero" up to the cancellation
    for name in ("db", "db_onepass"):
        assert float((r[name] - db).abs().max()) <= 1e-11 * float(r["M_db"].max())
    assert (r["M_dw"] >= r["dw"].abs()).all() and (r["M_P"] >= r["P"].abs()).all()


def test_two_shards_with_the_whole_batch_count_sum_to_the_whole_batch():
    B, T0, F0, C = 4, 11, 9, 16
    g = SO.gen(6)
    x = SO.logmel_like(g, (B, T0, F0), F64)
    w, b = rnd(g, 3, 3, 1, C, scale=0.3), rnd(g, C, scale=0.1)
    T1, F1, _, _ = SO.dims(T0, F0)
    N = B * T1 * F1
    fin = SO.finalize(SO.stats(SO.conv1(x, w, b)[0])["stats"], N, 1.0 + rnd(g, C, scale=0.2), rnd(g, C, scale=0.1))
    dy = rnd(g, B, T1, F1, C, scale=0.5)
    whole = SO.bn0_backward(x, w, b, fin, dy, N, N)
    halves = [SO.bn0_backward(x[s], w, b, fin, dy[s], N, N // 2, bstats=whole["bstats"]) for s in (slice(0, 2), slice(2, 4))]
    torch.testing.assert_close(halves[0]["bstats"] + halves[1]["bstats"], whole["bstats"], rtol=0, atol=1e-11)
    top = float(whole["dw"].abs().max())
    for name in ("dw", "dw_onepass"):
        assert float((halves[0][name] + halves[1][name] - whole["dw"]).abs().max()) <= 1e-11 * top
    for name in ("db", "db_onepass"):
        assert float((halves[0][name] + halves[1][name]).abs().max()) <= 1e-11 * float(whole["M_db"].max())
        assert float(halves[0][name].abs().max()) > 1e-3  # ... although neither half is zero on its own


SPARSE = [(name, dt) for name in SO.BN0_CASES for dt in (torch.float32, torch.bfloat16)]


@pytest.mark.parametrize("name,dtype", SPARSE, ids=lambda v: str(v).replace("torch.", ""))
def test_the_bounds_of_the_sparse_cases_see_one_lost_or_doubled_position(name, dtype):
    """For every position the sparse gradient lives on: the sums with that position left out, and with it counted twice, lie outside the
    bound the GPU test applies to bstats, pbuf and the two-pass dw (s0 / s1 are inputs of that kernel: the same bstats in all three)."""
    i = SO.bn0_inputs(name, dtype, "sparse")
    full = SO.bn0_backward(i["x"], i["w"], i["b"], i["fin"], i["dy"], i["count"])
    bs = full["bstats"].float()
    full = SO.bn0_backward(i["x"], i["w"], i["b"], i["fin"], i["dy"], i["count"], bstats=bs)
    bound = SO.bn0_backward_bounds(full)
    C = full["P"].shape[1]
    worst = float("inf")
    assert len(i["pos"]) >= 4
    for pos in i["pos"]:
        for factor in (0.0, 2.0):
            dy = i["dy"].double().clone()
            dy[pos] *= factor
            assert float(i["dy"][pos].abs().min()) > 0
            r = SO.bn0_backward(i["x"], i["w"], i["b"], i["fin"], dy, i["count"], bstats=bs)
            for what, got, want in (("bstats", r["bstats"], full["bstats"]), ("pbuf", torch.cat([r["P"].reshape(-1), r["bstats"][:C]]),
                                                                              torch.cat([full["P"].reshape(-1), full["bstats"][:C]])),
                                    ("dw", r["dw"], full["dw"])):
                ratio = float(((got - want).abs() / bound[what].reshape(got.shape)).max())
                worst = min(worst, ratio)
                assert ratio > 1, f"{what}: position {pos} x {factor} moves the sums by {ratio:.3g} of the bound only"
    print(f"{name}: a lost / doubled position is at least {worst:.3g} x the bound")
