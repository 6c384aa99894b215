"""float64 restatements of Conv2dSubsampling's pieces (csrc/conv2d.hip), CPU only.  None of them calls the library; test_subsampling_oracle.py
checks them against torch autograd and oracle/conformer_ref.py.

    conv1   Conv2D(filters, 3, strides 2, padding='causal') on a [B, T0, F0] feature map (Cin = 1): left pad 2 in time AND frequency, then
            VALID (subsampling.py:163-254, convolution.py:25-37,132-144); kernel keras-style [3, 3, 1, C], tap k = kh * 3 + kw
    BN0     keras BatchNormalization(momentum .99, epsilon 1e-3) + swish around conv1, given as fin = [mean | rstd | scale | shift]
    S       the haloed space-to-depth layout [B, T2+1, F2+1, 2, 2, C] of a [B, T1, F1, C] activation: element (b, t, f) sits in row
            (b, t/2 + 1, f/2 + 1), parity block (t%2, f%2); row 0 / column 0 of every sample (the halo) and the slots past an odd T1 / F1
            hold no element
    conv2   the same convolution with Cin = C, through torch.nn.functional.conv2d in float64 (autograd gives its gradients)

Every function takes the values the kernel is given (already rounded to their storage type) and returns float64.  The M_* entries are the
sum of |term| the bounds of test_conv2d_gpu.py are stated on.  A quantity that is RECOMPUTED from the feature map counts by the terms it is
formed from: z by its nine products and the bias (M_z), xhat = (z - mean) rstd by (M_z + |mean|) rstd, and swish'(u) = s + s u (1 - s) by
its two terms (it passes through zero at u = -1.278), as in norm_oracle.py."""
import torch
import torch.nn.functional as F

GRAM_N = 91  # G [9][9], s [9], N


def _d(a):
    return None if a is None else torch.as_tensor(a).detach().to("cpu", torch.float64)


def dims(T0, F0):
    """T1, F1 (conv1's output), T2, F2 (conv2's output = the S layout's rows): ceil(L / 2) each"""
    T1, F1 = (T0 + 1) // 2, (F0 + 1) // 2
    return T1, F1, (T1 + 1) // 2, (F1 + 1) // 2


def swish(z):
    return z * torch.sigmoid(z)


def dswish(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


# ------------------------------------------------------------------------------------------------------------------------- conv1
def patches(x):
    """[B, 9, T1, F1]: p_k(b, t, f) = x[b, 2t + kh - 2, 2f + kw - 2], zero outside, k = kh * 3 + kw"""
    x = _d(x)
    B, T0, F0 = x.shape
    T1, F1, _, _ = dims(T0, F0)
    xp = torch.zeros(B, 2 * T1 + 2, 2 * F1 + 2, dtype=torch.float64)  # index + 2; one spare row / column when T0 / F0 is odd
    xp[:, 2:2 + T0, 2:2 + F0] = x
    return torch.stack([xp[:, kh:kh + 2 * T1:2, kw:kw + 2 * F1:2] for kh in range(3) for kw in range(3)], 1)


def _wb(w, b):
    w = _d(w)
    w = w.reshape(9, w.shape[-1])
    return w, (torch.zeros(w.shape[1], dtype=torch.float64) if b is None else _d(b))


def conv1(x, w, b=None):
    """z [B, T1, F1, C] = b + sum_k w[k] p_k, and M_z = |b| + sum_k |w[k] p_k|"""
    p = patches(x)
    w, b = _wb(w, b)
    return torch.einsum("bktf,kc->btfc", p, w) + b, torch.einsum("bktf,kc->btfc", p.abs(), w.abs()) + b.abs()


def conv1_weight_grad(x, dy):
    """dw [9, C] = sum_pos p_k dy_c, db [C] = sum_pos dy_c, for a dense dy [B, T1, F1, C]"""
    p, dy = patches(x), _d(dy)
    return dict(dw=torch.einsum("bktf,btfc->kc", p, dy), db=dy.sum((0, 1, 2)),
                M_dw=torch.einsum("bktf,btfc->kc", p.abs(), dy.abs()), M_db=dy.abs().sum((0, 1, 2)))


def gram(x):
    """the 91 numbers [G (9 x 9) | s (9) | N]: G = sum_pos p p^T, s = sum_pos p, N = B T1 F1"""
    p = patches(x)
    return torch.cat([torch.einsum("batf,bctf->ac", p, p).reshape(81), p.sum((0, 2, 3)), torch.tensor([float(p[:, 0].numel())], dtype=torch.float64)])


def stats(z, M_z=None):
    """stats [2C] = (sum_pos z, sum_pos z^2) of a [..., C] tensor; M with z counted by M_z (default |z|)"""
    z = _d(z)
    z = z.reshape(-1, z.shape[-1])
    m = z.abs() if M_z is None else _d(M_z).reshape(z.shape)
    return dict(stats=torch.cat([z.sum(0), (z * z).sum(0)]), M_stats=torch.cat([m.sum(0), (m * m).sum(0)]))


def stats_from_gram(g, w, b=None):
    """sum z_c = W_c.s + N b_c,  sum z_c^2 = W_c^T G W_c + 2 b_c W_c.s + N b_c^2"""
    g = _d(g)
    w, b = _wb(w, b)
    G, s, N = g[:81].reshape(9, 9), g[81:90], g[90]
    ws = s @ w
    wgw = torch.einsum("kc,kl,lc->c", w, G, w)
    aws = s.abs() @ w.abs()
    return dict(stats=torch.cat([ws + N * b, wgw + 2 * b * ws + N * b * b]),
                M_stats=torch.cat([aws + N * b.abs(), torch.einsum("kc,kl,lc->c", w.abs(), G.abs(), w.abs()) + 2 * b.abs() * aws + N * b * b]))


def finalize(st, count, gamma, beta, eps=1e-3):
    """fin [4C] = mean, rstd, scale = gamma rstd, shift = beta - mean scale from stats = (sum z, sum z^2), as tfasr_bn_finalize (training)"""
    st, g, b = _d(st), _d(gamma), _d(beta)
    C = g.numel()
    mean = st[:C] / count
    var = (st[C:2 * C] / count - mean * mean).clamp_min(0)
    rstd = (var + float(torch.tensor(eps, dtype=torch.float32))) ** -0.5
    return torch.cat([mean, rstd, g * rstd, b - mean * g * rstd])


def _fin(fin):
    fin = _d(fin)
    C = fin.numel() // 4
    return fin[:C], fin[C:2 * C], fin[2 * C:3 * C], fin[3 * C:]


def bn0_apply(x, w, b, fin):
    """y = swish(conv1(x) scale + shift), dense [B, T1, F1, C]; M_y = M_z |scale| + |shift| (|swish'| <= 1.1)"""
    z, M_z = conv1(x, w, b)
    _, _, sc, sh = _fin(fin)
    return dict(y=swish(z * sc + sh), M_y=M_z * sc.abs() + sh.abs())


def bn0_backward(x, w, b, fin, dy, count, n_local=None, bstats=None):
    """The closed form above conv1_gram_kernel, with the `fin` it is handed; dy dense [B, T1, F1, C]:
        dz = dy swish'(z scale + shift),  xhat = (z - mean) rstd,  bstats = (sum dz, sum dz xhat)  (of THIS shard)
        s0, s1 = bstats / count  (`bstats` given: the all-reduced sums of every shard, else this shard's own)
        d = scale (dz - s0 - xhat s1),  dw = sum_pos p d,  db = sum_pos d  (two-pass route: sums of p_k d_c)
        P[k, c] = sum_pos p_k dz_c; one-pass route: dw = scale (P - s0 s - s1 X), X[k, c] = rstd ((G W_c)_k + (b_c - mean_c) s_k),
        db = scale (sum dz - s0 N - s1 rstd (W_c.s + N (b_c - mean_c))) with G, s, N = n_local of this shard - the same numbers.
    n_local (this shard's B T1 F1) is checked against x; `count` is the whole batch's."""
    p = patches(x)
    z, M_z = conv1(x, w, b)
    mean, rstd, sc, sh = _fin(fin)
    dy = _d(dy)
    N = z[..., 0].numel()
    assert n_local is None or n_local == N
    u = z * sc + sh
    s = torch.sigmoid(u)
    dz = dy * dswish(u)
    M_dz = dy.abs() * s * (1 + u.abs() * (1 - s))
    xh, M_xh = (z - mean) * rstd, (M_z + mean.abs()) * rstd
    own = torch.cat([dz.sum((0, 1, 2)), (dz * xh).sum((0, 1, 2))])
    M_bstats = torch.cat([M_dz.sum((0, 1, 2)), (M_dz * M_xh).sum((0, 1, 2))])
    bs = own if bstats is None else _d(bstats)
    C = mean.numel()
    s0, s1 = bs[:C] / count, bs[C:] / count
    d = sc * (dz - s0 - xh * s1)
    M_d = sc.abs() * (M_dz + s0.abs() + M_xh * s1.abs())
    P = torch.einsum("bktf,btfc->kc", p, dz)
    one = bn0_finalize(gram(x), w, b, fin, bs, count, torch.cat([P.reshape(-1), own[:C]]))
    return dict(dz=dz, bstats=own, M_bstats=M_bstats, P=P, M_P=torch.einsum("bktf,btfc->kc", p.abs(), M_dz), d=d,
                dw=torch.einsum("bktf,btfc->kc", p, d), db=d.sum((0, 1, 2)),
                M_dw=torch.einsum("bktf,btfc->kc", p.abs(), M_d), M_db=M_d.sum((0, 1, 2)),
                dw_onepass=one["dw"], db_onepass=one["db"], M_dw_onepass=one["M_dw"], M_db_onepass=one["M_db"])


def bn0_finalize(g, w, b, fin, bstats, count, pbuf):
    """tfasr_conv1_bn_bwd_finalize on the numbers it is handed: g [91] and pbuf = [P (9 x C) | sum dz (C)] of THIS shard, bstats and count of
    the whole batch.  dw [9, C] = scale (P - s0 s - s1 X), db = scale (sum dz - s0 N - s1 rstd (W.s + N (b - mean)))"""
    g, bs, pbuf = _d(g), _d(bstats), _d(pbuf)
    wk, bk = _wb(w, b)
    mean, rstd, sc, _ = _fin(fin)
    C = mean.numel()
    G, sv, N = g[:81].reshape(9, 9), g[81:90], g[90]
    P, sdz = pbuf[:9 * C].reshape(9, C), pbuf[9 * C:10 * C]
    s0, s1 = bs[:C] / count, bs[C:] / count
    X = rstd * (G @ wk + (bk - mean) * sv[:, None])
    M_X = rstd * (G.abs() @ wk.abs() + (bk.abs() + mean.abs()) * sv.abs()[:, None])
    return dict(dw=sc * (P - s0 * sv[:, None] - s1 * X), db=sc * (sdz - s0 * N - s1 * rstd * (sv @ wk + N * (bk - mean))),
                M_dw=sc.abs() * (P.abs() + (s0 * sv[:, None]).abs() + s1.abs() * M_X),
                M_db=sc.abs() * (sdz.abs() + (s0 * N).abs() + s1.abs() * rstd * (sv.abs() @ wk.abs() + N * (bk.abs() + mean.abs()))))


# ---------------------------------------------------------------------------------------------------------------------- the S layout
def valid_mask(B, T1, F1):
    """bool [B, T2+1, F2+1, 2, 2]: the slots that hold an element"""
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    m = torch.zeros(B, T2 + 1, F2 + 1, 2, 2, dtype=torch.bool)
    for pt in range(2):
        for pf in range(2):
            m[:, 1:1 + (T1 - pt + 1) // 2, 1:1 + (F1 - pf + 1) // 2, pt, pf] = True
    return m


def to_s2d(dense, fill=0.0):
    """[B, T1, F1, C] -> [B, T2+1, F2+1, 2, 2, C] (same dtype), `fill` in every slot that holds no element"""
    B, T1, F1, C = dense.shape
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    s = torch.full((B, T2 + 1, F2 + 1, 2, 2, C), fill, dtype=dense.dtype)
    for pt in range(2):
        for pf in range(2):
            sub = dense[:, pt::2, pf::2]
            s[:, 1:1 + sub.shape[1], 1:1 + sub.shape[2], pt, pf] = sub
    return s


def from_s2d(s, T1, F1):
    """the [B, T1, F1, C] elements of an S-layout tensor"""
    B, C = s.shape[0], s.shape[-1]
    s = s.reshape(B, (T1 + 1) // 2 + 1, (F1 + 1) // 2 + 1, 2, 2, C)
    dense = torch.empty(B, T1, F1, C, dtype=s.dtype)
    for pt in range(2):
        for pf in range(2):
            sub = dense[:, pt::2, pf::2]
            sub.copy_(s[:, 1:1 + sub.shape[1], 1:1 + sub.shape[2], pt, pf])
    return dense


# ------------------------------------------------------------------------------------------------------------------- im2col / conv2
def im2col(x):
    """[B, T1, F1, C] -> [B T2 F2, 9 C]: col[(b, t2, f2), k C + c] = x[b, 2 t2 + kh - 2, 2 f2 + kw - 2, c], zero outside"""
    x = _d(x)
    B, T1, F1, C = x.shape
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    xp = torch.zeros(B, 2 * T2 + 2, 2 * F2 + 2, C, dtype=torch.float64)
    xp[:, 2:2 + T1, 2:2 + F1] = x
    return torch.stack([xp[:, kh:kh + 2 * T2:2, kw:kw + 2 * F2:2] for kh in range(3) for kw in range(3)], 3).reshape(B * T2 * F2, 9 * C)


def col2im(dcol, B, T1, F1, C):
    """the adjoint of im2col: dx[b, t1, f1, c] = sum of dcol[(b, t2, f2), k C + c] over the (t2, f2, k) that read (t1, f1)"""
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    dcol = _d(dcol).reshape(B, T2, F2, 9, C)
    dxp = torch.zeros(B, 2 * T2 + 2, 2 * F2 + 2, C, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            dxp[:, kh:kh + 2 * T2:2, kw:kw + 2 * F2:2] += dcol[:, :, :, kh * 3 + kw]
    return dxp[:, 2:2 + T1, 2:2 + F1].contiguous()


def conv2(x1, W, b, dy=None):
    """y [B, T2, F2, C] of the causal 3x3 stride-2 convolution with W [9 Cin, Cout] (keras [3, 3, Cin, Cout] flattened); with dy also its
    gradients dx1, dW [9 Cin, Cout], db by torch autograd, all float64"""
    x1, W, b = _d(x1).requires_grad_(dy is not None), _d(W).requires_grad_(dy is not None), _d(b).requires_grad_(dy is not None)
    Cin, Cout = x1.shape[-1], W.shape[-1]
    xp = F.pad(x1.permute(0, 3, 1, 2), (2, 0, 2, 0))
    y = F.conv2d(xp, W.reshape(3, 3, Cin, Cout).permute(3, 2, 0, 1), b, stride=2).permute(0, 2, 3, 1)
    if dy is None:
        return y
    y.backward(_d(dy))
    return dict(y=y.detach(), dx=x1.grad, dW=W.grad, db=b.grad)


# ------------------------------------------------------------------------------- inputs shared by the CPU and the GPU tests of BatchNorm0
# The backward grids are min(B T1, max(64, resident blocks)), and no more than CUs x (threads per CU) / 256 blocks of 256 threads can be
# resident: 256 x 2048 / 256 on an MI355X.  With twice that many rows plus one, every block makes a second trip whatever the occupancy
# query returned (test_conv2d_gpu.py checks the device's own numbers against this constant).
MAX_RESIDENT_BLOCKS = 256 * 2048 // 256
BN0_CASES = {                       # B, T0, F0, C
    "c8_few_rows": (2, 9, 7, 8),            # B T1 = 10 < 64 blocks; F1 = 4 < the 256 (apply: 8 channels a thread) / 128 (backward: 4) f sub-lanes
    "c144_idle_lanes": (3, 11, 20, 144),    # C / 8 = 18, C / 4 = 36: 252 of 256 threads live in both
    "c256": (2, 50, 17, 256),               # odd F1 = 9, F0 odd
    "c64_even": (3, 37, 80, 64),            # even F1 = 40, odd T1 = 19
    "two_trips": (3, 2 * ((2 * MAX_RESIDENT_BLOCKS + 1 + 2) // 3) - 1, 9, 16),  # B T1 = 3 x 1366 = 4098 >= 2 x 2048 + 1
}
assert 3 * dims(BN0_CASES["two_trips"][1], 9)[0] >= 2 * MAX_RESIDENT_BLOCKS + 1


def gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(int(s) for s in seed)) % (2 ** 31))


def logmel_like(g, shape, dtype):
    """log-mel like features: mean^2 >> variance"""
    return (torch.randn(*shape, generator=g) * 2.5 - 6.0).to(dtype)


def sparse_positions(B, T1, F1):
    """the handful of (b, t, f) a sparse gradient lives on: first / last t, first / last f, both parities of each, the last sample, and (the
    last rows of the last sample) a row its block reaches on its second trip"""
    pos = [(0, 0, 0), (0, 0, F1 - 1), (0, T1 - 1, 0), (B - 1, T1 - 1, F1 - 1), (B - 1, min(1, T1 - 1), min(1, F1 - 1)),
           (B - 1, max(T1 - 2, 0), max(F1 - 2, 0)), (B - 1, T1 - 1, min(1, F1 - 1))]
    return sorted(set(pos))


def bn0_inputs(name, dtype, kind):
    """x (dtype), w, b, fin (float32; the float64 batch statistics of conv1(x), finalized and rounded) and a dense dy (dtype): Gaussian
    (`random`) or zero outside sparse_positions (`sparse`)"""
    B, T0, F0, C = BN0_CASES[name] if isinstance(name, str) else name
    g = gen(21, B, T0, F0, C)
    x = logmel_like(g, (B, T0, F0), dtype)
    w, b = torch.randn(3, 3, 1, C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    z, _ = conv1(x, w, b)
    T1, F1, _, _ = dims(T0, F0)
    fin = finalize(stats(z)["stats"], B * T1 * F1, gamma, beta).float()
    dy = (torch.randn(B, T1, F1, C, generator=g) * 0.5).to(dtype)
    pos = sparse_positions(B, T1, F1)
    if kind == "sparse":
        keep = torch.zeros(B, T1, F1, 1, dtype=torch.bool)
        for p in pos:
            keep[p] = True
        dy = torch.where(keep, dy, torch.zeros((), dtype=dtype))
    return dict(x=x, w=w, b=b, fin=fin, dy=dy, pos=pos, count=B * T1 * F1)


K_ELEM, K_SUM, K_BF16 = 2.0 ** -20, 2.0 ** -18, 2.0 ** -8  # the constants of test_norm_gpu.py
# tfasr_conv1_stats_from_gram / _bn_bwd_finalize work in double and round ONCE to float32: an ulp of the result (and of the destination it
# is added to), plus, in the finalize, the float32 rounding of 1 / count that s0 and s1 carry: 4 u of the terms; the double arithmetic over
# < 200 terms stays below 2^-44 of them
K_FINALIZE, K_DOUBLE = 2.0 ** -22, 2.0 ** -44


def bn0_backward_bounds(ref):
    """the absolute bounds test_conv2d_gpu.py applies to the outputs of the BatchNorm0 backward kernels, each on the terms that route sums
    in float32: bstats (both routes), pbuf = [P | sum dz] (one pass), dw / db (two passes)"""
    C = ref["P"].shape[1]
    return dict(bstats=K_SUM * ref["M_bstats"], pbuf=K_SUM * torch.cat([ref["M_P"].reshape(-1), ref["M_bstats"][:C]]),
                dw=K_SUM * ref["M_dw"], db=K_SUM * ref["M_db"])
