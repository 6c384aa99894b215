"""tests/norm_oracle.py (the float64 reference of the csrc/norm.hip tests) against torch autograd on the expressions of
oracle/conformer_ref.py, in float64, at one small shape.  Runs without a GPU."""
import numpy as np
import torch

import norm_oracle as NO
from oracle import conformer_ref as R

ROWS, C = 13, 24


def _rand(seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    return dict(x=r(ROWS, C) * 1.5 + 0.3, dy=r(ROWS, C), add=r(ROWS, C), gamma=r(C), beta=r(C) * 0.1, mm=r(C), mv=torch.rand(C, generator=g, dtype=torch.float64) + 0.5)


def close(a, b):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-11, atol=1e-12)


def test_layernorm_against_autograd():
    d = _rand()
    x, g, b = (d[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = R.layer_norm(x, g, b, eps=float(np.float32(1e-3)))
    y.backward(d["dy"])
    f = NO.layernorm_fwd(d["x"], d["gamma"], d["beta"])
    close(f["y"], y)
    close(f["mean"], d["x"].mean(-1))
    close(f["rstd"], torch.rsqrt(d["x"].var(-1, unbiased=False) + float(np.float32(1e-3))))
    for add in (None, d["add"]):
        bw = NO.layernorm_bwd(d["dy"], d["x"], d["gamma"], f["mean"], f["rstd"], add=add)
        close(bw["dx"], x.grad + (0 if add is None else add))
        close(bw["dgamma"], g.grad)
        close(bw["dbeta"], b.grad)
        assert (bw["M_dx"] >= bw["dx"].abs() - 1e-12).all() and (bw["M_dgamma"] >= bw["dgamma"].abs()).all() and (bw["M_dbeta"] >= bw["dbeta"].abs()).all()
    assert (f["M_y"] >= f["y"].abs() - 1e-12).all() and (f["M_mean"] >= f["mean"].abs()).all()


def test_layernorm_eps_is_the_float32_value():
    """(1e-3 in float32 is 0.001000000047...: at zero variance the difference is 2.4e-8 relative in rstd, above a float64 comparison)"""
    x = torch.full((1, C), 0.25, dtype=torch.float64)
    f = NO.layernorm_fwd(x, torch.ones(C), torch.zeros(C))
    assert abs(float(f["rstd"][0]) / float(np.float32(1e-3)) ** -0.5 - 1) < 1e-14
    assert abs(float(f["rstd"][0]) / 1e-3 ** -0.5 - 1) > 1e-8


def _bn(d, act):
    x, g, b = (d[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y, mean, var = R.batch_norm_train(x, g, b, eps=float(np.float32(1e-3)))
    if act:
        y = R.swish(y)
    y.backward(d["dy"])
    return x, g, b, y, mean, var


def test_batchnorm_training_against_autograd():
    d = _rand(1)
    mom = float(np.float32(0.99))
    for act in (False, True):
        x, g, b, y, mean, var = _bn(d, act)
        mo = NO.bn_moments(d["x"])
        close(mo["stats"][:C], d["x"].sum(0))
        close(mo["stats"][C:], (d["x"] ** 2).sum(0))
        f = NO.bn_finalize(mo["stats"], ROWS, d["gamma"], d["beta"], d["mm"], d["mv"])
        close(f["mean"], mean)
        close(f["var"], var)
        close(f["fin"][C:2 * C], torch.rsqrt(var + float(np.float32(1e-3))))
        close(f["moving_mean"], d["mm"] * mom + mean * (1 - mom))
        close(f["moving_var"], d["mv"] * mom + var * (1 - mom))
        close(NO.bn_apply(d["x"], f["fin"], act)["y"], y)
        s = NO.bn_bwd_sums(d["x"], d["dy"], f["fin"], act)
        close(s["bstats"][:C], b.grad)
        close(s["bstats"][C:], g.grad)
        bw = NO.bn_bwd_apply(d["x"], d["dy"], f["fin"], s["bstats"], ROWS, act)
        close(bw["dx"], x.grad)
        assert (bw["M_dx"] >= bw["dx"].abs() - 1e-12).all() and (s["M_bstats"] >= s["bstats"].abs()).all()


def test_batchnorm_inference_uses_the_moving_statistics_and_leaves_them():
    d = _rand(2)
    f = NO.bn_finalize(None, 1, d["gamma"], d["beta"], d["mm"], d["mv"], training=False)
    close(NO.bn_apply(d["x"], f["fin"])["y"], R.batch_norm_infer(d["x"], d["gamma"], d["beta"], d["mm"], d["mv"], eps=float(np.float32(1e-3))))
    assert torch.equal(f["moving_mean"], d["mm"]) and torch.equal(f["moving_var"], d["mv"])
    bnd = NO.bn_finalize_bounds(f, None, 1, d["gamma"], d["beta"], d["mm"], d["mv"], training=False)
    assert float(bnd["mean"].max()) == 0 and float(bnd["rstd"].max()) < 1e-5


def test_finalize_bounds_hold_for_a_float32_evaluation():
    """the propagated bounds of bn_finalize_bounds hold (with room) for numpy's float32 evaluation of the same one-pass formulas"""
    g = torch.Generator().manual_seed(3)
    rows = 4000
    x = (torch.randn(rows, C, generator=g) * 1.5 + 0.3).float()
    gam, bet = (torch.rand(C, generator=g) + 0.5).float(), (torch.randn(C, generator=g) * 0.1).float()
    mm0, mv0 = torch.randn(C, generator=g).float(), (torch.rand(C, generator=g) + 0.5).float()
    mo = NO.bn_moments(x)
    f = NO.bn_finalize(mo["stats"], rows, gam, bet, mm0, mv0)
    bnd = NO.bn_finalize_bounds(f, mo["M_stats"], rows, gam, bet, mm0, mv0)
    xn = x.numpy()
    s0, s1 = np.zeros(C, np.float32), np.zeros(C, np.float32)
    for r in range(rows):  # fully sequential float32 sums
        s0 += xn[r]
        s1 += xn[r] * xn[r]
    n, e, mom = np.float32(rows), np.float32(1e-3), np.float32(0.99)
    mean = s0 / n
    var = np.maximum(s1 / n - mean * mean, np.float32(0))
    rstd = (np.float32(1) / np.sqrt(var + e)).astype(np.float32)
    scale = gam.numpy() * rstd
    shift = bet.numpy() - mean * scale
    got = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, moving_mean=mm0.numpy() * mom + mean * (np.float32(1) - mom),
               moving_var=mv0.numpy() * mom + var * (np.float32(1) - mom))
    for k, v in got.items():
        err = (torch.from_numpy(v).double() - f[k]).abs()
        assert (err <= bnd[k]).all(), k
        assert (bnd[k] <= 1e-4 * (1 + f[k].abs())).all(), k  # ... and are no licence: 1e-4 relative at the most
