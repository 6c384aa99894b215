"""LayerNorm and BatchNorm, forward and backward, restated plainly in float64 torch on the CPU: what the kernels of csrc/norm.hip must
compute.  The GPU tests (tests/test_norm_gpu.py) hold every launch branch of that file to these functions; tests/test_norm_oracle.py pins
them against torch autograd on the expressions of oracle/conformer_ref.py (layer_norm, batch_norm_train, swish).

Follows  keras.layers.LayerNormalization(epsilon=1e-3)                      encoders/conformer.py:59-64,101-109
         keras.layers.BatchNormalization(momentum=.99, epsilon=1e-3) + swish  encoders/conformer.py:327-342, subsampling.py:197-214

Every function takes the values the kernel is given (already rounded to its storage type) and returns a dict of float64 tensors: the
results, and under "M_<name>" the magnitude sums the rounding bounds of the tests are stated in:
    elementwise outputs   M = sum of |term| over the terms that form the element
    sums over rows        M = sum over rows of |term|, per column
`eps` and `momentum` enter as the float32 values the C ABI passes."""
import numpy as np
import torch

LN_EPS = 1e-3
BN_EPS = 1e-3
BN_MOMENTUM = 0.99
U = 2.0 ** -24  # unit roundoff of float32


def _d(a):
    return None if a is None else torch.as_tensor(a).detach().to("cpu", torch.float64)


def _f32(v):
    return float(np.float32(v))


def swish(z):
    return z * torch.sigmoid(z)


def dswish(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


# ------------------------------------------------------------------------------------ LayerNorm
def layernorm_fwd(x, gamma, beta, eps=LN_EPS):
    """x [rows, C] -> y, mean [rows], rstd [rows] (biased variance).  The terms of x - mean are x and the row's x / C."""
    x, g, b = _d(x), _d(gamma), _d(beta)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = (var + _f32(eps)) ** -0.5
    y = (x - mean[:, None]) * rstd[:, None] * g + b
    mabs = x.abs().mean(-1)
    return dict(y=y, mean=mean, rstd=rstd, M_y=(x.abs() + mabs[:, None]) * rstd[:, None] * g.abs() + b.abs(), M_mean=mabs, M_rstd=rstd)


def layernorm_bwd(dy, x, gamma, mean, rstd, add=None):
    """dx = add + rstd * (dy g - s1 - xhat s2), s1 = mean_c(dy g), s2 = mean_c(dy g xhat); dgamma = sum_rows dy xhat; dbeta = sum_rows dy.
    mean / rstd [rows] are inputs (what the forward saved).  M_dx counts s1 and s2 by the terms THEY are formed from, mean_c |dy g| and
    mean_c |dy g xhat|: their rounding error is an ulp of those, however close to zero the two means themselves come out."""
    dy, x, g, m, rs, add = _d(dy), _d(x), _d(gamma), _d(mean), _d(rstd), _d(add)
    xh = (x - m[:, None]) * rs[:, None]
    dg = dy * g
    s1 = dg.mean(-1, keepdim=True)
    s2 = (dg * xh).mean(-1, keepdim=True)
    dx = rs[:, None] * (dg - s1 - xh * s2)
    a1 = dg.abs().mean(-1, keepdim=True)
    a2 = (dg * xh).abs().mean(-1, keepdim=True)
    M = rs[:, None] * (dg.abs() + a1 + xh.abs() * a2)
    if add is not None:
        dx = dx + add
        M = M + add.abs()
    return dict(dx=dx, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), M_dx=M, M_dgamma=(dy * xh).abs().sum(0), M_dbeta=dy.abs().sum(0))


# ------------------------------------------------------------------------------------ BatchNorm
def bn_moments(x):
    """stats [2C] = (sum_rows x, sum_rows x^2)"""
    x = _d(x)
    x = x.reshape(-1, x.shape[-1])
    return dict(stats=torch.cat([x.sum(0), (x * x).sum(0)]), M_stats=torch.cat([x.abs().sum(0), (x * x).sum(0)]))


def bn_finalize(stats, count, gamma, beta, moving_mean=None, moving_var=None, momentum=BN_MOMENTUM, eps=BN_EPS, training=True):
    """fin [4C] = mean, rstd, scale = gamma rstd, shift = beta - mean scale.  Training: mean / biased variance of the batch from `stats`,
    and moving = moving momentum + batch (1 - momentum); inference: the moving statistics, left as they are."""
    g, b, mm, mv = _d(gamma), _d(beta), _d(moving_mean), _d(moving_var)
    C = g.numel()
    mom = _f32(momentum)
    if training:
        s = _d(stats)
        mean = s[:C] / count
        var = (s[C:] / count - mean * mean).clamp_min(0)
        if mm is not None:
            mm = mm * mom + mean * (1 - mom)
        if mv is not None:
            mv = mv * mom + var * (1 - mom)
    else:
        mean, var = mm, mv
    rstd = (var + _f32(eps)) ** -0.5
    scale = g * rstd
    shift = b - mean * scale
    return dict(fin=torch.cat([mean, rstd, scale, shift]), mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, moving_mean=mm, moving_var=mv)


def bn_finalize_bounds(f, M_stats, count, gamma, beta, moving_mean=None, moving_var=None, momentum=BN_MOMENTUM, eps=BN_EPS, training=True,
                       k_sum=2.0 ** -18, k_var=2.0 ** -16):
    """Absolute bounds on a float32 evaluation of bn_finalize (result `f`), propagated from the two the sums give:
        |d mean| <= k_sum * sum|x| / n        |d var| <= k_var * (mean^2 + var)      (through S1 / n - (S0 / n)^2)
    rstd between its values at var -+ d var (+ 4 ulp for rsqrt), scale = gamma rstd, shift = beta - mean scale, the moving statistics
    through their update; every float32 operation adds an ulp of its operands.  `moving_*` are the values BEFORE the update."""
    g, b, mm0, mv0 = _d(gamma), _d(beta), _d(moving_mean), _d(moving_var)
    C = g.numel()
    e, mom = _f32(eps), _f32(momentum)
    mean, var, rstd, scale = f["mean"], f["var"], f["rstd"], f["scale"]
    if training:
        dmean = k_sum * _d(M_stats)[:C] / count + 2 * U * mean.abs()
        dvar = k_var * (mean * mean + var)
    else:
        dmean, dvar = torch.zeros_like(mean), torch.zeros_like(var)
    lo, hi = ((var - dvar).clamp_min(0) + e) ** -0.5, (var + dvar + e) ** -0.5
    drstd = torch.maximum((lo - rstd).abs(), (hi - rstd).abs()) + 4 * U * rstd
    dscale = g.abs() * drstd + 2 * U * scale.abs()
    dshift = dmean * scale.abs() + mean.abs() * dscale + 4 * U * (b.abs() + (mean * scale).abs())
    out = dict(mean=dmean, var=dvar, rstd=drstd, scale=dscale, shift=dshift, fin=torch.cat([dmean, drstd, dscale, dshift]))
    if training and mm0 is not None:
        out["moving_mean"] = (1 - mom) * dmean + 4 * U * ((mm0 * mom).abs() + (mean * (1 - mom)).abs())
        out["moving_var"] = (1 - mom) * dvar + 4 * U * ((mv0 * mom).abs() + (var * (1 - mom)).abs())
    return out


def _fin(fin):
    fin = _d(fin)
    C = fin.numel() // 4
    return fin[:C], fin[C:2 * C], fin[2 * C:3 * C], fin[3 * C:]


def bn_apply(x, fin, act_swish=False):
    """y = act(x scale + shift)"""
    x = _d(x)
    _, _, sc, sh = _fin(fin)
    z = x * sc + sh
    return dict(y=swish(z) if act_swish else z, M_y=(x * sc).abs() + sh.abs())


def _dz(x, dy, sc, sh, act_swish):
    """dz = dy act'(z), and the magnitude of its terms: swish'(z) = s + s z (1 - s) passes through zero at z = -1.278, where an ulp of its
    two terms is no longer an ulp of their sum"""
    if not act_swish:
        return dy, dy.abs()
    z = x * sc + sh
    s = torch.sigmoid(z)
    return dy * dswish(z), dy.abs() * s * (1 + z.abs() * (1 - s))


def bn_bwd_sums(x, dy, fin, act_swish=False):
    """bstats [2C] = (sum_rows dz, sum_rows dz xhat), dz = dy act'(x scale + shift), xhat = (x - mean) rstd: dbeta and dgamma"""
    x, dy = _d(x), _d(dy)
    x, dy = x.reshape(-1, x.shape[-1]), dy.reshape(-1, x.shape[-1])
    mean, rstd, sc, sh = _fin(fin)
    dz, _ = _dz(x, dy, sc, sh, act_swish)
    t = dz * (x - mean) * rstd
    return dict(bstats=torch.cat([dz.sum(0), t.sum(0)]), M_bstats=torch.cat([dz.abs().sum(0), t.abs().sum(0)]))


def bn_bwd_apply(x, dy, fin, bstats, count, act_swish=False):
    """dx = scale (dz - S0 / n - xhat S1 / n).  The terms of xhat are x rstd and mean rstd (the row kernel multiplies them out)."""
    x, dy, bs = _d(x), _d(dy), _d(bstats)
    mean, rstd, sc, sh = _fin(fin)
    C = mean.numel()
    s0, s1 = bs[:C] / count, bs[C:] / count
    dz, mdz = _dz(x, dy, sc, sh, act_swish)
    dx = sc * (dz - s0 - (x - mean) * rstd * s1)
    return dict(dx=dx, M_dx=sc.abs() * (mdz + s0.abs() + (x.abs() + mean.abs()) * rstd * s1.abs()))
