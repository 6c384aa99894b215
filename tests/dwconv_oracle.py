"""The causal depthwise convolution and the GLU around it, forward and backward, restated plainly in float64 torch on the CPU (closed form, no
autograd): what the kernels of csrc/dwconv.hip and the scalar / GLU kernels of csrc/elementwise.hip must compute.  The GPU tests
(tests/test_dwconv_gpu.py) hold every launch branch to these functions; tests/test_dwconv_oracle.py pins them against torch autograd on
oracle/conformer_ref.depthwise_conv1d_causal and a * sigmoid(b).

Follows  DepthwiseConv1D(padding="causal")   layers/convolution.py:159-228, encoders/conformer.py:305-313
         GLU over the last axis             activations/glu.py:25-28

Every function takes the values the kernel is given (already rounded to its storage type) and returns a dict of float64 tensors: the
results, and under "M_<name>" the magnitude sums the rounding bounds of the tests are stated in, as tests/norm_oracle.py does:
    elementwise outputs   M = sum of |term| over the terms that form the element
    sums over rows        M = sum over rows of |term|, per column

Where the kernels round (csrc/dwconv.hip; all accumulation between these points is float32):
    GIN    g = a sigmoid(b) is rounded to bf16 (pack2_bf16, line 154) before it enters LDS: the taps see the rounded g (what is stored to
           gx_out, line 159)
    BNIN   dcv = sc dz + cb x + cd is rounded to bf16 (pack2_bf16, line 226) before it enters LDS: the taps see the rounded dcv (what is
           stored to bn.dcv, line 230)
    STATS  the sums are taken of the bf16-ROUNDED y (the packed pair `pk` is unpacked again, lines 269-275)
    GLU    the data gradient dx stays in float32 registers (acc, line 266-267): it is NOT rounded before da / db are formed
    y / dx / dglu are rounded to bf16 once, when they are stored; dw / dbias / stats / dgamma / dbeta are float32 sums
The chained quantities of the fused kernels (y of GIN from g, dglu of BNIN from dcv, stats from y) are therefore restated from the ROUNDED
intermediate: the GPU tests pass the intermediate the kernel stored (itself held to this file) into the next function."""
import torch

import norm_oracle as NO

TGD = 16  # output steps per thread group of the forward / data-gradient tile kernel: a workgroup owns 2 TGD = 32 steps


def _d(a):
    return None if a is None else torch.as_tensor(a).detach().to("cpu", torch.float64)


def dwconv_fwd(x, w, bias=None):
    """x [B, T, C], w [K, C], bias [C] | None:  y[b,t,c] = bias[c] + sum_k w[k,c] x[b,t-(K-1)+k,c], zero outside [0, T) per utterance"""
    x, w, bias = _d(x), _d(w), _d(bias)
    B, T, C = x.shape
    K = w.shape[0]
    xp = torch.cat([torch.zeros(B, K - 1, C, dtype=torch.float64), x], 1)
    y, M = torch.zeros_like(x), torch.zeros_like(x)
    for k in range(K):
        t = w[k] * xp[:, k:k + T]
        y, M = y + t, M + t.abs()
    if bias is not None:
        y, M = y + bias, M + bias.abs()
    return dict(y=y, M_y=M)


def dwconv_bwd_data(dy, w):
    """dx[b,t,c] = sum_k w[k,c] dy[b,t+(K-1)-k,c]"""
    dy, w = _d(dy), _d(w)
    B, T, C = dy.shape
    K = w.shape[0]
    dp = torch.cat([dy, torch.zeros(B, K - 1, C, dtype=torch.float64)], 1)
    dx, M = torch.zeros_like(dy), torch.zeros_like(dy)
    for k in range(K):
        t = w[k] * dp[:, K - 1 - k:K - 1 - k + T]
        dx, M = dx + t, M + t.abs()
    return dict(dx=dx, M_dx=M)


def dwconv_bwd_weight(x, dy, K):
    """dw[k,c] = sum_{b,t} dy[b,t,c] x[b,t-(K-1)+k,c]; dbias[c] = sum_{b,t} dy[b,t,c]"""
    x, dy = _d(x), _d(dy)
    B, T, C = x.shape
    xp = torch.cat([torch.zeros(B, K - 1, C, dtype=torch.float64), x], 1)
    dw, M = torch.zeros(K, C, dtype=torch.float64), torch.zeros(K, C, dtype=torch.float64)
    for k in range(K):
        t = dy * xp[:, k:k + T]
        dw[k], M[k] = t.sum((0, 1)), t.abs().sum((0, 1))
    return dict(dw=dw, dbias=dy.sum((0, 1)), M_dw=M, M_dbias=dy.abs().sum((0, 1)))


def glu_fwd(x2c):
    """x2c [..., 2C] = a | b:  g = a sigmoid(b)"""
    x2c = _d(x2c)
    C = x2c.shape[-1] // 2
    g = x2c[..., :C] * torch.sigmoid(x2c[..., C:])
    return dict(g=g, M_g=g.abs())


def glu_bwd(x2c, dg, M_dg=None):
    """d [..., 2C] = da | db:  da = dg sigmoid(b), db = dg a sigmoid(b) (1 - sigmoid(b)).  M_dg: the magnitude of dg's own terms, where dg
    is a sum the same kernel formed (the data gradient in front of the fused GLU backward); |dg| otherwise.
    The terms of db are dg a s and dg a s^2: the kernels form 1 - s from the float32 s, so for b >> 0, where 1 - s is small, an ulp of s
    (2^-24) is no longer an ulp of 1 - s, and the rounding error of db is an ulp of dg a s, not of db (as norm_oracle._dz counts swish')."""
    x2c, dg = _d(x2c), _d(dg)
    C = x2c.shape[-1] // 2
    a, s = x2c[..., :C], torch.sigmoid(x2c[..., C:])
    m = dg.abs() if M_dg is None else _d(M_dg)
    fa, fb = s, a * s * (1 - s)
    return dict(d=torch.cat([dg * fa, dg * fb], -1), M_d=torch.cat([m * fa, m * a.abs() * s * (1 + s)], -1))


def bn_stats_of(y):
    """stats [2C] = per channel the sum and the sum of squares of the given (bf16) values, all rows of all utterances"""
    return NO.bn_moments(y)


def stats_copy_of(B, T, ncopy, tile=2 * TGD):
    """[B, number of time tiles]: the copy the workgroup of (utterance b, time tile j) adds into, (j + b) % ncopy"""
    nt = (T + tile - 1) // tile
    return (torch.arange(nt)[None, :] + torch.arange(B)[:, None]) % ncopy


def bn_stats_copies(y, ncopy, tile=2 * TGD):
    """stats [ncopy, 2C]: the statistics of y [B, T, C] as the forward kernel spreads them: the rows of (time tile j, utterance b) land
    in copy (j + b) % ncopy.  M_stats likewise."""
    y = _d(y)
    B, T, C = y.shape
    cp = stats_copy_of(B, T, ncopy, tile)
    st, M = torch.zeros(ncopy, 2 * C, dtype=torch.float64), torch.zeros(ncopy, 2 * C, dtype=torch.float64)
    for b in range(B):
        for j in range(cp.shape[1]):
            m = NO.bn_moments(y[b, j * tile:(j + 1) * tile])
            st[cp[b, j]] += m["stats"]
            M[cp[b, j]] += m["M_stats"]
    return dict(stats=st, M_stats=M)


def bn_bwd_prologue(bn_x, dsw, fin, bstats, count):
    """The BatchNorm-with-swish backward the BNIN variant forms while it stages: dcv = norm_oracle.bn_bwd_apply(..., swish), the arithmetic
    of bn_apply_bwd_rows_kernel, from the sums bstats [copies, 2C] added up over the copies."""
    bs = _d(bstats).reshape(-1, 2 * bn_x.shape[-1]).sum(0)
    r = NO.bn_bwd_apply(bn_x, dsw, fin, bs, count, act_swish=True)
    return dict(dcv=r["dx"], M_dcv=r["M_dx"], bsum=bs)
