"""One tfasr_gemm call restated plainly in float64 torch on the CPU, the dispatcher's choice of kernel restated in plain Python, and the
table of cases that pins every route of csrc/gemm.hip, csrc/gemm_fast.hip and csrc/gemm_big.h (tests/test_gemm_routes_gpu.py runs it on the
GPU; tests/test_gemm_oracle.py checks this file on the CPU; tests/test_gemm_route.py holds route() against the library's own answer).

reference()  the terms in the order the epilogue of gemm_kernel (csrc/gemm.hip) defines:
                 v = alpha * acc + bias;  prez = v;  v = act(v);  v *= dact(dact_z);  v = keep ? v / (1 - p) : 0;  v = res + beta * v;
                 D = v   (accumulate: D = start + v);  colsum = colsum_start + alpha * sum_k B[k, :]
             The dropout mask `keep` is an argument: the hash is not restated here.  Operands, dact_z, res and keep are FLAT buffers read
             through the strides of the call, exactly as the kernels read them.
route()      what gemm_route() of csrc/gemm_route.h chooses for a call on a part with `cus` compute units, restated independently.  A test
             asserts the label its case was written for (and the launch count), so on a part where the rule picks another kernel the test
             fails instead of testing something else.
library_route() / label_of()   the same answer from the library itself (tfasr_gemm_route), brought to a label: tests/test_gemm_route.py
             holds the two against each other on the CPU, tests/test_gemm_routes_gpu.py at the live CU count.
gemm_args()  the tfasr_gemm_args of a case as kernels._gemm_args fills them, over FAKE addresses (the route looks at null-ness and
             alignment only).
cases()      the case table, with M sized from the CU count wherever the route depends on it.

Labels   ("fast", 64 | 128, "persist" | "one", epilogue)   gemm_fast_kernel / gemm_fast_one_kernel <TA, TB, BN, EPI>
         ("big", 256 | 320, "0" | "E_DACT", "tr" | "rows")  gemm_big_kernel (256-row tiles; tr = transposed accumulators in the epilogue)
         ("generic", "bf16" | "f32", 64 | 128)              gemm_kernel<T, TA, TB, BN>
         ("generic+colsum", "bf16" | "f32", 64 | 128)       tfasr_colsum, then gemm_kernel (two launches)
         ("group", 128, "E_CSUM") / ("one by one",)         tfasr_gemm_group
         ("seg", 128) / ("ktab", 128, "E_CSUM") / ("big-seg", 256, "0", "tr" | "rows") / ("status", 1 | 3)   route_full() only
route_full() restates the ROUTE (status, kernel, launch count) of calls with K-segments, row_tiles, k_tiles, lse, rgrad, bns and the split-K
workspace as well; their results stay out of scope here (their own tests), as do ffn_fused and dense_ln."""
import math
from dataclasses import dataclass, replace

import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd._lib import ACT_FACTOR, ACT_NONE, ACT_SIGMOID, ACT_SWISH, ACT_TANH, ACT_TANH_OUT

F64 = torch.float64
NAN = float("nan")
U23 = 2.0 ** -23
K_BF16 = 2.0 ** -8          # bf16 output: round-to-nearest moves a value by at most half an ulp = 2^-8 of it
ELEM_RTOL, ELEM_ATOL = 1e-5, 1e-6   # the suite's element bound for swish, tanh, sigmoid and their derivatives (test_pointwise_gpu._elem_bound)
LIPSCHITZ = {ACT_NONE: 1.0, ACT_SWISH: 1.1, ACT_TANH: 1.0, ACT_SIGMOID: 0.25}  # sup |act'|
NONLINEAR_DACT = (ACT_SWISH, ACT_TANH, ACT_SIGMOID)
GUARD = 24  # elements behind the last one a buffer's view reaches


def ceil_div(a, b):
    return -(-a // b)


def up8(n):
    return (n + 7) & ~7


# ---------------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    name: str
    label: tuple
    M: int
    N: int
    K: int
    ta: bool = False
    tb: bool = False
    dtype: str = "bf16"      # storage type of A, B, res, dact_z, prez (and of D unless out_f32)
    out_f32: bool = False
    lda: int = 0             # 0: the smallest stride the fast path takes (bf16: the row length rounded up to 8)
    ldb: int = 0
    ldd: int = 0             # 0: N
    nb1: int = 1
    nb2: int = 1             # batches: contiguous operands per batch, D at sD2 = M * ldd + 1 (an odd offset) when nb1 * nb2 > 1
    a_off: int = 0           # elements the operand starts into its (256-byte aligned) buffer
    b_off: int = 0
    d_off: int = 0           # the same for D, res, dact_z and prez
    alpha: float = 1.0
    beta: float = 1.0
    bias: bool = False
    prez: bool = False
    res: bool = False
    act: int = ACT_NONE
    dact: int = ACT_NONE     # != NONE: the call has a dact_z
    drop_p: float = 0.0      # exact kind; the random kind runs p = 0.1
    accumulate: bool = False
    split_k: int = 1
    colsum: bool = False
    kinds: tuple = ("exact", "random")
    launches: int = 1
    # the optional parts of the struct that only the route is restated for (route_full(); their results have tests of their own)
    seg_k: int = 0           # != 0: the call has a seg_a_off table with this seg_k
    row_tiles: int = 0       # != 0: a row-tile table with this n_row_tiles
    k_tiles: int = 0         # != 0: a K-block table with this n_k_tiles
    lse: int = 0             # 1: lse_part / row_label / pick with lse_parts = ceil(N / 128) * 2; 2: with lse_parts one too many
    no_D: bool = False       # D is NULL
    rgrad: bool = False      # rgrad_coef and row_label
    bns: bool = False        # bns_out / bns_x / bns_fin, channels bns_c
    bns_c: int = 0
    ws: bool = False         # a split-K workspace that is large enough

    # ---- what the struct of the call holds
    @property
    def f32(self):
        return self.dtype == "f32"

    @property
    def d_f32(self):
        return self.f32 or self.out_f32

    @property
    def a_shape(self):  # as stored
        return (self.K, self.M) if self.ta else (self.M, self.K)

    @property
    def b_shape(self):
        return (self.N, self.K) if self.tb else (self.K, self.N)

    @property
    def nb(self):
        return self.nb1 * self.nb2

    @property
    def sA(self):
        s = self.a_shape[0] * self.lda
        return (self.nb2 * s, s) if self.nb > 1 else (0, 0)

    @property
    def sB(self):
        s = self.b_shape[0] * self.ldb
        return (self.nb2 * s, s) if self.nb > 1 else (0, 0)

    @property
    def sD(self):
        s = self.M * self.ldd + 1
        return (self.nb2 * s, s) if self.nb > 1 else (0, 0)

    @property
    def nonlinear(self):
        return self.act != ACT_NONE or self.dact in NONLINEAR_DACT

    def a_len(self):
        return self.a_off + (self.nb - 1) * self.sA[1] + (self.a_shape[0] - 1) * self.lda + up8(self.a_shape[1]) + GUARD

    def b_len(self):
        return self.b_off + (self.nb - 1) * self.sB[1] + (self.b_shape[0] - 1) * self.ldb + up8(self.b_shape[1]) + GUARD

    def d_len(self):
        return self.d_off + (self.nb - 1) * self.sD[1] + self.M * self.ldd + self.ldd + GUARD  # one guard row and a tail


def mk(name, label, M, N, K, **kw):
    c = Case(name, tuple(label), M, N, K, **kw)
    pad = (lambda n: n) if c.f32 else up8
    return replace(c, lda=c.lda or pad(c.a_shape[1]), ldb=c.ldb or pad(c.b_shape[1]), ldd=c.ldd or N)


def a_view(c, flat):
    """op(A) [nb1, nb2, M, K] of the flat operand buffer"""
    r, k = (1, c.lda) if c.ta else (c.lda, 1)
    return flat.as_strided((c.nb1, c.nb2, c.M, c.K), (c.sA[0], c.sA[1], r, k), c.a_off)


def b_view(c, flat):
    """op(B) [nb1, nb2, K, N]"""
    k, n = (1, c.ldb) if c.tb else (c.ldb, 1)
    return flat.as_strided((c.nb1, c.nb2, c.K, c.N), (c.sB[0], c.sB[1], k, n), c.b_off)


def d_view(c, flat):
    """[nb1, nb2, M, N] of a flat buffer addressed like D (res, dact_z, prez; the dropout mask, whose index 0 is the element D points at)"""
    return flat.as_strided((c.nb1, c.nb2, c.M, c.N), (c.sD[0], c.sD[1], c.ldd, 1), c.d_off)


# ------------------------------------------------------------------------------------------------------------------ the reference
def act_f(v, act):
    if act == ACT_SWISH:
        return v * torch.sigmoid(v)
    if act == ACT_TANH:
        return torch.tanh(v)
    if act == ACT_SIGMOID:
        return torch.sigmoid(v)
    assert act == ACT_NONE
    return v


def dact_f(z, dact):
    if dact == ACT_SWISH:
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if dact == ACT_TANH:
        return 1 - torch.tanh(z) ** 2
    if dact == ACT_SIGMOID:
        s = torch.sigmoid(z)
        return s * (1 - s)
    if dact == ACT_TANH_OUT:
        return 1 - z * z
    assert dact == ACT_FACTOR
    return z


def reference(c, A, B, bias=None, dact_z=None, keep=None, drop_p=0.0, res=None, start=None, colsum_start=None, want_S=True, sum_exact=False):
    """c: the Case (shapes, strides, alpha / beta / act / dact / accumulate / colsum).  A, B, dact_z, res, keep (bool), start: FLAT buffers
    (any dtype; values already rounded to the storage type), bias [N], colsum_start [N].  Returns float64 tensors:
      D [nb1, nb2, M, N], prez (= alpha acc + bias), colsum [N] (when c.colsum),
      S = sum_k |alpha a_ik b_kj| + |bias_j| (+ |start|), S_colsum, and
      E = the error a correct kernel may leave in D: (K + 2) 2^-23 S through the chain (0 when sum_exact), the element bound of every
          non-linear function, one f32 rounding per further multiply / add.  E_prez likewise.  Without a bf16 term (see bound())."""
    d = lambda t: None if t is None else t.detach().to("cpu", F64)
    a, b = a_view(c, d(A)), b_view(c, d(B))
    alpha, beta = float(torch.tensor(c.alpha, dtype=torch.float32)), float(torch.tensor(c.beta, dtype=torch.float32))
    acc = torch.matmul(a, b)
    v = alpha * acc
    del acc
    bias = d(bias)
    if bias is not None:
        v = v + bias
    out = {}
    if sum_exact:
        S, E = None, torch.zeros(())
    else:
        S = abs(alpha) * torch.matmul(a.abs(), b.abs())
        if bias is not None:
            S = S + bias.abs()
        E = (c.K + 2) * U23 * S
    out["prez"], out["E_prez"] = v, E
    if c.act != ACT_NONE:
        v = act_f(v, c.act)
        E = LIPSCHITZ[c.act] * E + ELEM_RTOL * v.abs() + ELEM_ATOL
    if c.dact != ACT_NONE:
        g = dact_f(d_view(c, d(dact_z)), c.dact)
        eg = (ELEM_RTOL * g.abs() + ELEM_ATOL) if c.dact in NONLINEAR_DACT else (U23 * (1 + g.abs()) if c.dact == ACT_TANH_OUT else 0.0)
        E = g.abs() * E + v.abs() * eg + U23 * (v * g).abs()
        v = v * g
    if keep is not None:
        p = float(torch.tensor(drop_p, dtype=torch.float32))
        kp = d_view(c, keep.detach().cpu())
        v = torch.where(kp, v / (1.0 - p), torch.zeros_like(v))
        E = torch.where(kp, E / (1.0 - p) + 2 * U23 * v.abs(), torch.zeros_like(v))  # 1 / (1 - p) rounded, then the product
    if res is not None:
        r = d_view(c, d(res))
        E = abs(beta) * E + U23 * (r.abs() + (beta * v).abs())
        v = r + beta * v
    if c.accumulate:
        s0 = d_view(c, d(start))
        v = s0 + v
        if not sum_exact:
            S = S + s0.abs()
            E = (c.K + 3) * U23 * S
    out["D"], out["E"] = v, E
    if want_S and S is not None:
        out["S"] = S
    if c.colsum:
        bs = b.reshape(c.K, c.N)
        out["colsum"] = d(colsum_start) + alpha * bs.sum(0)
        out["S_colsum"] = d(colsum_start).abs() + abs(alpha) * bs.abs().sum(0)
        out["E_colsum"] = torch.zeros(()) if sum_exact else (c.K + 2) * U23 * out["S_colsum"]
    return out


def bound(E, ref, bf16):
    """E of reference(); a bf16 output adds the rounding of the f32 value, which is within E of ref: 2^-8 (|ref| + E)"""
    return E * (1 + K_BF16) + K_BF16 * ref.abs() if bf16 else E + torch.zeros_like(ref)


# --------------------------------------------------------------------------------------------------------------------- the inputs
def _gen(c, kind):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(c.name + kind)) % (2 ** 31))


def _ints(g, n, lim, step=1.0):
    return torch.randint(-lim, lim + 1, (n,), generator=g).float() * step


def _place(flat, view_of, vals):
    view_of(flat).copy_(vals)
    return flat


def make_inputs(c, kind):
    """CPU float32 tensors holding values of the storage type (the caller casts, which is then exact): flat A and B with NaN in every
    element the product must not use, bias, flat dact_z / res / start laid out like D, colsum_start; alpha / drop_p of this kind in the
    returned Case.  exact: operands integers in [-3, 3], bias and res multiples of 1/4, FACTOR / TANH_OUT inputs multiples of 1/8 in
    [-1, 1], the arguments of the non-linear derivatives multiples of 1/8 in [-8, 8], start values multiples of 1/4.  random: Gaussian."""
    g = _gen(c, kind)
    st = torch.float32 if c.f32 else torch.bfloat16
    rt = lambda t: t.to(st).float()
    exact = kind == "exact"
    sh = (c.nb1, c.nb2)
    lg = max(0, math.ceil(math.log2(math.sqrt(c.K))))
    if exact:
        alpha = 2.0 ** -lg if c.act != ACT_NONE else 0.5   # act(z): z = alpha acc + bias mostly inside [-8, 8] (std <= 4)
        av = _ints(g, c.nb * c.M * c.K, 3).view(*sh, c.M, c.K)
        bv = _ints(g, c.nb * c.K * c.N, 3).view(*sh, c.K, c.N)
        drop_p = c.drop_p
    else:
        alpha = 2.0 ** -lg
        av = rt(torch.randn(*sh, c.M, c.K, generator=g))
        bv = rt(torch.randn(*sh, c.K, c.N, generator=g))
        drop_p = 0.1 if c.drop_p > 0 else 0.0
    c = replace(c, alpha=alpha, beta=0.25 if c.res else 1.0, drop_p=drop_p)
    x = dict(A=_place(torch.full((c.a_len(),), NAN), lambda f: a_view(c, f), av),
             B=_place(torch.full((c.b_len(),), NAN), lambda f: b_view(c, f), bv))
    del av, bv
    nd = c.nb * c.M * c.N
    dflat = lambda vals: _place(torch.full((c.d_len(),), NAN), lambda f: d_view(c, f), vals.view(*sh, c.M, c.N))
    if c.bias:
        x["bias"] = _ints(g, c.N, 8, 0.25) if exact else torch.randn(c.N, generator=g)  # (f32 in every mode)
    if c.dact != ACT_NONE:
        if c.dact in NONLINEAR_DACT:
            z = _ints(g, nd, 64, 0.125) if exact else rt(torch.randn(nd, generator=g) * 3)
        elif c.dact == ACT_TANH_OUT:
            z = _ints(g, nd, 8, 0.125) if exact else rt(torch.tanh(torch.randn(nd, generator=g)))
        else:
            z = _ints(g, nd, 8, 0.125) if exact else rt(torch.randn(nd, generator=g))
        x["dact_z"] = dflat(z)
    if c.res:
        x["res"] = dflat(_ints(g, nd, 16, 0.25) if exact else rt(torch.randn(nd, generator=g)))
    if c.accumulate:
        x["start"] = dflat(_ints(g, nd, 8, 0.25) if exact else torch.randn(nd, generator=g))
    if c.colsum:
        x["colsum_start"] = _ints(g, c.N, 8, 0.25) if exact else torch.randn(c.N, generator=g)
    return c, x


def largest_partial_sum(c, x):
    """an upper bound of every partial sum of |a b| (and of the column sums) of the case: K max|a| max|b|"""
    a, b = a_view(c, x["A"]), b_view(c, x["B"])
    return c.K * float(a.abs().max()) * max(float(b.abs().max()), 1.0)


# ---------------------------------------------------------------------------------------------------------------------- the route
E_NAMES = {0: "0", 1: "E_ACT", 5: "E_ACT|E_DROP", 2: "E_DACT", 6: "E_DACT|E_DROP", 8: "E_RES", 12: "E_RES|E_DROP", 1024: "E_MUL"}
E_ACT, E_DACT, E_DROP, E_RES, E_MUL = 1, 2, 4, 8, 1024
INF = 1 << 40


def _fast_refusal(c):
    """why the bf16 LDS-DMA kernels hand the call back to the generic ones (None: they take it)"""
    if c.f32:
        return "dtype"
    if c.a_off % 8 or c.b_off % 8:  # (buffers start on 256 bytes)
        return "operand off 16 bytes"
    if c.lda % 8 or c.ldb % 8:
        return "ld % 8"
    if any(s % 8 for s in c.sA + c.sB):
        return "batch stride % 8"
    if c.ta and up8(c.M) > c.lda:
        return "trans_a: 16-byte chunks leave the row"
    if not c.tb and up8(c.N) > c.ldb:
        return "B: 16-byte chunks leave the row"
    if c.K < 8:
        return "K < 8"
    return None


def _launch_epi(c, bn, epi, tiles, cus):
    if bn == 64 and epi not in ("E_CSUM", "E_WS", "E_LSE") and c.split_k <= 1 and tiles > 2 * cus:
        return ("fast", 64, "one", epi)
    return ("fast", bn, "persist", epi)


def _launch_big(c, generic, need, tanh_out, cus):
    """the 256-row kernels of gemm_big.h (None: not eligible)"""
    if generic or need or c.accumulate or c.split_k > 1 or c.nb != 1 or c.colsum or c.out_f32 or c.K < 128 or c.K % 8 or c.M < 256 or (c.tb and c.N % 8):
        return None
    seg = c.seg_k != 0
    if seg and not (c.seg_k > 0 and c.seg_k % 64 == 0 and c.K % c.seg_k == 0 and c.K // 64 <= 64):
        return None
    if c.tb and not seg and not c.lse and c.N % 320 == 0:
        bn = 320
    elif c.N >= (256 if c.tb else 192) and (c.N % 256 == 0 or c.N % 256 >= 192):
        bn = 256
    else:
        return None
    if ceil_div(c.N, bn) * ceil_div(c.M, 256) < 2 * cus:
        return None
    if tanh_out and (not c.tb or seg or c.lse):
        return None
    if c.lse and not (bn == 256 and c.lse == 1):
        return None
    if c.rgrad and (c.tb or seg or tanh_out or bn != 256):
        return None
    if c.no_D and not c.lse:
        return None
    tr = c.ldd % 8 == 0 and c.N % 8 == 0 and (c.no_D or c.d_off % 8 == 0)
    if tanh_out:
        return ("big", bn, "E_DACT", "tr" if (tr and bn == 256) else "rows")
    if bn == 320:
        return ("big", bn, "0", "rows")
    if c.lse:  # (the statistics kernel has no K-segment variant: a table that came this far is ignored)
        return None if c.tb else ("big", 256, "E_LSE", "tr" if (tr or c.no_D) else "rows")
    if c.rgrad:
        return ("big", 256, "E_RGRAD", "rows")
    return ("big-seg" if seg else "big", bn, "0", "tr" if tr else "rows")


def _launch_one(c, cus):
    """the bf16 kernels of gemm_fast.hip / gemm_big.h (None: left to the generic ones)"""
    split = max(c.split_k, 1)
    if c.k_tiles:  # K-block table: the accumulating x^T dy product on 128-wide tiles, or nothing
        ok = (c.ta and not c.tb and c.accumulate and c.nb == 1 and not c.ws and not c.seg_k and not c.row_tiles and not c.lse and not c.rgrad and
              not c.bns and 0 < c.k_tiles <= ceil_div(c.K, 256) and c.d_f32)
        return ("ktab", 128, "E_CSUM") if ok else None
    t128 = ceil_div(c.N, 128) * ceil_div(c.M, 128) * c.nb * split
    lim = INF if (split <= 1 and not c.accumulate and not c.colsum and min(c.K, c.N) <= 256) else cus
    narrow = not c.lse and not c.seg_k and (c.N <= 64 or (t128 <= lim and not (c.accumulate and c.ws)))
    bn = 64 if narrow else 128
    tiles = ceil_div(c.N, bn) * ceil_div(c.M, 128) * c.nb * split
    need, generic = 0, False
    dz = c.dact != ACT_NONE
    if not c.accumulate:
        generic = c.out_f32
        if c.act != ACT_NONE or c.prez:
            if c.act == ACT_SWISH:
                need |= E_ACT
            else:
                generic = True
        if dz:
            if c.dact == ACT_SWISH:
                need |= E_DACT
            elif c.dact == ACT_FACTOR:
                need |= E_MUL
            else:
                generic = True
        if c.drop_p > 0:
            need |= E_DROP
        if c.res:
            need |= E_RES
    plain = not generic and need == 0
    if c.bns:  # BatchNorm sums in the epilogue: the plain NT product on 64-column tiles, or nothing
        ok = (not c.ta and c.tb and narrow and plain and not c.accumulate and not c.bias and split == 1 and c.nb == 1 and c.N % 8 == 0 and c.ldd % 8 == 0 and
              (c.bns_c == 0 or (c.bns_c > 0 and c.bns_c % 8 == 0 and c.N % c.bns_c == 0)) and c.d_off % 8 == 0 and not c.no_D and
              not c.colsum and not c.lse and not c.seg_k and not c.rgrad)
        return _launch_epi(c, 64, "E_BNS", tiles, cus) if ok else None
    if not c.ta:
        tanh_out = not c.accumulate and dz and c.dact == ACT_TANH_OUT
        other = c.out_f32 or c.act != ACT_NONE or c.prez or (dz and not tanh_out)
        big = _launch_big(c, other, need, tanh_out, cus)
        if big:
            return big
    if c.rgrad or c.no_D:  # gradient epilogue / statistics-only projection: 256-row kernel only
        return None
    if c.accumulate and split > 1 and c.nb == 1 and c.ws and not narrow and not c.colsum:
        return ("fast", 128, "persist", "E_WS")
    if c.colsum:
        if c.ta and not c.tb and c.accumulate and c.N > 64:
            return _launch_epi(c, bn, "E_CSUM", tiles, cus)
        return None
    nn, nt = not c.ta and not c.tb, not c.ta and c.tb
    if c.seg_k:  # K-segments: the plain NN / NT product on 128-wide tiles, without statistics
        ok = (not c.ta and plain and not c.accumulate and split == 1 and c.nb == 1 and c.seg_k > 0 and c.seg_k % 64 == 0 and c.K % c.seg_k == 0 and
              c.K // 64 <= 64 and not c.lse)
        return ("seg", 128) if ok else None
    if c.lse:
        ok = nn and plain and not c.accumulate and c.nb == 1 and c.lse == 1
        return ("fast", 128, "persist", "E_LSE") if ok else None
    if not generic:
        compiled = need == 0 or (nn and need in (E_RES, E_RES | E_DROP))
        if not narrow or (t128 > cus and c.N > 64):
            compiled = compiled or (nn and need in (E_ACT, E_ACT | E_DROP)) or (nt and need in (E_DACT, E_DACT | E_DROP, E_MUL))
        if compiled:
            return _launch_epi(c, bn, E_NAMES[need], tiles, cus)
    return _launch_epi(c, bn, "E_GEN", tiles, cus)


def route(c, cus):
    """the kernel tfasr_gemm launches for the call `c` on a part with `cus` compute units"""
    label = None if _fast_refusal(c) else _launch_one(c, cus)
    if label:
        return label
    tiles = ceil_div(c.N, 128) * ceil_div(c.M, 128) * c.nb * max(c.split_k, 1)  # the generic kernels of gemm.hip
    width = 64 if (c.f32 and c.N > 64 and tiles < 2 * cus) else 128
    return ("generic+colsum" if c.colsum else "generic", c.dtype, width)


def route_full(c, cus):
    """(label, launches) of ANY call, the optional tables / statistics / gradient epilogue / BatchNorm sums / workspace included, restated from
    tfasr_gemm as it stood before csrc/gemm_route.h; a refused call gives (("status", 1 | 3), None)"""
    INVALID, UNSUPPORTED = (("status", 1), None), (("status", 3), None)
    split = max(c.split_k, 1)
    if (c.no_D and not c.lse) or (c.rgrad and (c.no_D or c.lse)) or min(c.M, c.N, c.K) <= 0:
        return INVALID
    if (c.accumulate and not c.d_f32) or (split > 1 and not c.accumulate):
        return INVALID
    if split > 1 and (c.res or c.dact != ACT_NONE or c.prez or c.act != ACT_NONE or c.drop_p > 0):
        return INVALID
    if not 0 <= c.drop_p < 1 or (c.colsum and not (c.accumulate and c.ta and not c.tb and c.nb == 1)):
        return INVALID
    if c.row_tiles:
        if c.row_tiles <= 0 or c.row_tiles > ceil_div(c.M, 256):
            return INVALID
        if not c.seg_k or c.ta or c.accumulate or split > 1 or c.nb != 1 or c.f32:
            return UNSUPPORTED
    if c.k_tiles:
        if c.k_tiles <= 0 or c.k_tiles > ceil_div(c.K, 256):
            return INVALID
        if not c.ta or c.tb or not c.accumulate or c.nb != 1 or c.f32 or c.seg_k or c.row_tiles or c.ws:
            return UNSUPPORTED
    label = None if _fast_refusal(c) else _launch_one(c, cus)
    if label:
        return label, (2 if label[-1] == "E_WS" else 1)
    if c.k_tiles or c.lse or c.rgrad or c.bns or c.seg_k:
        return UNSUPPORTED
    label = route(c, cus)
    return label, (2 if c.colsum else 1)


def route_group(cs, cus):
    """tfasr_gemm_group on a list of at most 10 calls"""
    ok = 2 <= len(cs) <= 10 and all(
        not c.f32 and c.ta and not c.tb and c.accumulate and c.nb == 1 and not (c.bias or c.res or c.prez) and c.dact == ACT_NONE and
        c.act == ACT_NONE and c.drop_p == 0 and not _fast_refusal(c) and up8(c.N) <= c.ldb and c.N > 64 for c in cs)
    if ok:  # units per XCD: (product, k-slice) pairs dealt onto the least loaded of 8 lists of at most 20
        total = sum(ceil_div(c.N, 128) * ceil_div(c.M, 128) for c in cs)
        split = max(1, 2 * cus // total)
        units = sum(min(64, max(1, min(split, c.K // 512))) for c in cs)
        ok = units <= 8 * 20 // 2  # (far from the list limit: the exact dealing is not restated)
    return ("group", 128, "E_CSUM") if ok else ("one by one",)


# ------------------------------------------------------------------------------------------------- the library's own answer
BASE = 0x7F0000000000  # a 256-byte aligned address nothing reads: operands, D, res, dact_z, prez each get a region of their own
REGION = 1 << 36
E_LABELS = {**E_NAMES, 16: "E_WS", 32: "E_CSUM", 64: "E_LSE", 128: "E_RGRAD", 256: "E_GEN", 512: "E_BNS"}


def gemm_args(c):
    """tfasr_gemm_args of the case as kernels._gemm_args fills them; every pointer = its region's base + the case's element offset"""
    esz, dsz = (4 if c.f32 else 2), (4 if c.d_f32 else 2)
    at = lambda region, off, size: BASE + region * REGION + off * size
    a = _lib.GemmArgs()
    a.A, a.B, a.D = at(0, c.a_off, esz), at(1, c.b_off, esz), at(2, c.d_off, dsz)
    a.bias = at(3, 0, 4) if c.bias else None
    a.res = at(4, c.d_off, esz) if c.res else None
    a.dact_z = at(5, c.d_off, esz) if c.dact != ACT_NONE else None
    a.prez = at(6, c.d_off, esz) if c.prez else None
    a.colsum = at(7, 0, 4) if c.colsum else None
    a.M, a.N, a.K, a.lda, a.ldb, a.ldd = c.M, c.N, c.K, c.lda, c.ldb, c.ldd
    a.trans_a, a.trans_b, a.nb1, a.nb2 = int(c.ta), int(c.tb), c.nb1, c.nb2
    (a.sA1, a.sA2), (a.sB1, a.sB2), (a.sD1, a.sD2) = c.sA, c.sB, c.sD
    a.alpha, a.beta, a.act, a.dact = c.alpha, c.beta, c.act, c.dact
    a.dtype = _lib.TFASR_F32 if c.f32 else _lib.TFASR_BF16
    a.out_f32, a.accumulate, a.split_k = int(c.d_f32), int(c.accumulate), c.split_k
    a.drop_p, a.drop_seed = c.drop_p, 1
    if c.no_D:
        a.D = None
    if c.seg_k:
        a.seg_a_off, a.seg_k = at(8, 0, 8), c.seg_k
    if c.row_tiles:
        a.row_tiles, a.n_row_tiles = at(9, 0, 4), c.row_tiles
    if c.k_tiles:
        a.k_tiles, a.n_k_tiles = at(10, 0, 4), c.k_tiles
    if c.lse:
        a.lse_part, a.row_label, a.pick, a.lse_parts = at(11, 0, 4), at(12, 0, 4), at(13, 0, 4), ceil_div(c.N, 128) * 2 + (c.lse - 1)
    if c.rgrad:
        a.rgrad_coef, a.row_label = at(14, 0, 4), at(12, 0, 4)
    if c.bns:
        a.bns_x, a.bns_fin, a.bns_out, a.bns_copies, a.bns_c = at(15, 0, esz), at(16, 0, 4), at(17, 0, 4), 1, c.bns_c
    if c.ws:
        a.ws, a.ws_elems = at(18, 0, 4), max(c.split_k, 1) * c.M * c.N
    return a


def label_of(info, c):
    """the label of a tfasr_gemm_route_info (None: a route outside the labels of this file)"""
    if info.status != 0:
        return ("status", info.status)
    if info.family in (_lib.GEMM_FAST_PERSISTENT, _lib.GEMM_FAST_ONE):
        return ("fast", info.tile_n, "persist" if info.family == _lib.GEMM_FAST_PERSISTENT else "one", E_LABELS.get(info.epi))
    if info.family == _lib.GEMM_BIG:
        return ("big-seg" if info.seg else "big", info.tile_n, E_LABELS.get(info.epi), "tr" if info.tr else "rows")
    if info.family == _lib.GEMM_FAST_SEG:
        return ("seg", info.tile_n)
    if info.family == _lib.GEMM_FAST_KTAB:
        return ("ktab", info.tile_n, E_LABELS.get(info.epi))
    if info.family == _lib.GEMM_GENERIC:
        return ("generic+colsum" if info.launches == 2 else "generic", c.dtype, info.tile_n)
    return None


def library_route(c, cus):
    """(label, launches) of the call `c` on `cus` compute units as tfasr_gemm_route gives them"""
    import ctypes

    info = _lib.GemmRouteInfo()
    st = _lib.load().tfasr_gemm_route(ctypes.byref(gemm_args(c)), cus, ctypes.byref(info))
    assert st == info.status
    return label_of(info, c), (info.launches if st == 0 else None)


def library_route_group(cs, cus):
    """the label of tfasr_gemm_group on the calls `cs` as tfasr_gemm_group_route counts its launches"""
    import ctypes

    arr = (_lib.GemmArgs * len(cs))(*[gemm_args(c) for c in cs])
    n = ctypes.c_int(-1)
    assert _lib.load().tfasr_gemm_group_route(arr, len(cs), cus, ctypes.byref(n)) == 0
    return ("group", 128, "E_CSUM") if n.value == ceil_div(len(cs), 10) else ("one by one",)


# ------------------------------------------------------------------------------------------------------------------ the case table
LAYOUTS = [("nn", False, False), ("nt", False, True), ("tn", True, False), ("tt", True, True)]
SMALL = [(200, 144, 136), (130, 40, 72), (77, 64, 64), (129, 200, 8)]
GROUP_SHAPES = [(1024, 256, 1000, True), (256, 1024, 1000, True), (256, 256, 1000, True), (256, 512, 1000, False), (256, 768, 1000, True),
                (256, 256, 150, False), (144, 576, 993, True), (200, 72, 1000, True)]


def _compiled(prefix, label3, M, N, K, out, which="all", **kw):
    """the compiled epilogues of launch_one on one shape: label3 = ("fast", bn, mode)"""
    rows = [("res", "E_RES", dict(bias=True, res=True)),
            ("res_drop", "E_RES|E_DROP", dict(bias=True, res=True, drop_p=0.5)),
            ("act", "E_ACT", dict(bias=True, prez=True, act=ACT_SWISH)),
            ("act_drop", "E_ACT|E_DROP", dict(bias=True, prez=True, act=ACT_SWISH, drop_p=0.75)),
            ("dact", "E_DACT", dict(tb=True, dact=ACT_SWISH)),
            ("dact_drop", "E_DACT|E_DROP", dict(tb=True, dact=ACT_SWISH, drop_p=0.5)),
            ("mul", "E_MUL", dict(tb=True, dact=ACT_FACTOR, bias=True))]
    for nm, epi, e in rows:
        if which == "all" or nm in which:
            out.append(mk(f"{prefix}-{nm}", label3 + (epi,), M, N, K, **{**e, **kw}))


def _generic_epilogues(prefix, label, M, N, K, out, **kw):
    """E_GEN: tanh / sigmoid, their derivatives, an f32 output, a pre-activation without swish, TANH_OUT"""
    out.append(mk(f"{prefix}-gen_tanh", label, M, N, K, bias=True, prez=True, act=ACT_TANH, res=True, **kw))
    out.append(mk(f"{prefix}-gen_sigmoid_drop", label, M, N, K, bias=True, act=ACT_SIGMOID, drop_p=0.5, **kw))
    out.append(mk(f"{prefix}-gen_f32_swish", label, M, N, K, bias=True, prez=True, act=ACT_SWISH, out_f32=True, **kw))
    out.append(mk(f"{prefix}-gen_f32_plain", label, M, N, K, bias=True, res=True, drop_p=0.75, out_f32=True, tb=True, **kw))
    out.append(mk(f"{prefix}-gen_prez_only", label, M, N, K, bias=True, prez=True, **kw))
    out.append(mk(f"{prefix}-gen_dtanh", label, M, N, K, tb=True, dact=ACT_TANH, **kw))
    out.append(mk(f"{prefix}-gen_dsigmoid", label, M, N, K, tb=True, dact=ACT_SIGMOID, res=True, **kw))
    out.append(mk(f"{prefix}-gen_dswish_f32", label, M, N, K, tb=True, dact=ACT_SWISH, out_f32=True, **kw))
    out.append(mk(f"{prefix}-gen_tanh_out", label, M, N, K, tb=True, dact=ACT_TANH_OUT, bias=True, drop_p=0.5, **kw))


def cases(cus):
    """name -> Case for a part with `cus` compute units (the names do not depend on cus)"""
    out = []
    P64, O64, P128 = ("fast", 64, "persist"), ("fast", 64, "one"), ("fast", 128, "persist")
    # ---- persist64: small products
    for M, N, K in SMALL:
        for ln, ta, tb in LAYOUTS:
            out.append(mk(f"p64-{M}x{N}x{K}-{ln}", P64 + ("0",), M, N, K, ta=ta, tb=tb, bias=(ln == "nt")))
    out.append(mk("p64-k77-lda80", P64 + ("0",), 200, 144, 77, lda=80))
    for M, N, K in SMALL[:2]:
        _compiled(f"p64-{M}x{N}x{K}", P64, M, N, K, out, which=("res", "res_drop"))
        _generic_epilogues(f"p64-{M}x{N}x{K}", P64 + ("E_GEN",), M, N, K, out)
    # the activation epilogues are compiled for 64-column tiles only above CUs 128-wide tiles: on a small product they run E_GEN
    out.append(mk("p64-small-act-is-gen", P64 + ("E_GEN",), 200, 144, 136, bias=True, prez=True, act=ACT_SWISH, drop_p=0.5))
    out.append(mk("p64-small-dact-is-gen", P64 + ("E_GEN",), 200, 144, 136, tb=True, dact=ACT_SWISH, drop_p=0.5))
    out.append(mk("p64-small-mul-is-gen", P64 + ("E_GEN",), 200, 144, 136, tb=True, dact=ACT_FACTOR))
    # ---- persist64 with the compiled activation epilogues: more than CUs 128-wide tiles, at most 2 CUs 64-wide ones
    Mp = 128 * (cus // 2 + 8) - 37
    _compiled("p64c", P64, Mp, 192, 136, out, which=("act", "act_drop", "dact", "dact_drop", "mul"))
    # ---- one64: more than 2 CUs 64-wide tiles
    Mo = 128 * (ceil_div(2 * cus, 3) + 2) - 37
    out.append(mk("o64-plain-nn", O64 + ("0",), Mo, 192, 136))
    out.append(mk("o64-plain-tn", O64 + ("0",), Mo, 192, 136, ta=True, bias=True))
    _compiled("o64", O64, Mo, 192, 136, out)
    _generic_epilogues("o64", O64 + ("E_GEN",), Mo, 192, 136, out)
    # ---- persist128: one tile per workgroup (384 % 256 = 128 keeps the 256-row tiles out, K = 320 = 5 slabs)
    M1 = 128 * (ceil_div(cus + 1, 3) + 1) - 37
    for ln, ta, tb in LAYOUTS:
        out.append(mk(f"p128-plain-{ln}", P128 + ("0",), M1, 384, 320, ta=ta, tb=tb, bias=(ln == "nn")))
    out.append(mk("p128-k333-lda344", P128 + ("0",), M1, 384, 333, lda=344))
    _compiled("p128", P128, M1, 384, 320, out)
    _generic_epilogues("p128", P128 + ("E_GEN",), M1, 384, 320, out)
    # ---- persist128, several tiles per workgroup (the cross-tile prefetch)
    out.append(mk("p128x-plain-nn", P128 + ("0",), Mo, 384, 320))
    out.append(mk("p128x-plain-nt", P128 + ("0",), Mo, 384, 320, tb=True, bias=True))
    _compiled("p128x", P128, Mo, 384, 320, out, which=("res_drop", "dact_drop"))
    # ---- weight gradients: TN, accumulate onto a start value, f32 output
    wg = dict(ta=True, accumulate=True, out_f32=True)
    for split in (1, 5, 8):
        out.append(mk(f"wg64-split{split}", P64 + ("0",), 144, 200, 1000, split_k=split, **wg))
        out.append(mk(f"wg64-split{split}-colsum", P64 + ("E_CSUM",), 144, 200, 1000, split_k=split, colsum=True, **wg))
    out.append(mk("wg128-split32", P128 + ("0",), 384, 384, 4096 + 40, split_k=32, **wg))
    out.append(mk("wg128-split32-colsum", P128 + ("E_CSUM",), 384, 384, 4096 + 40, split_k=32, colsum=True, **wg))
    out.append(mk("wg-n48-colsum", ("generic+colsum", "bf16", 128), 144, 48, 1000, split_k=5, colsum=True, launches=2, **wg))
    out.append(mk("wg-f32-colsum", ("generic+colsum", "f32", 64), 144, 200, 1000, split_k=5, colsum=True, launches=2, dtype="f32", **wg))
    # ---- 256-row tiles: the smallest eligible products
    Mb = 256 * 2 * cus + 77
    out.append(mk("big256-nn", ("big", 256, "0", "tr"), Mb, 256, 128, bias=True))
    out.append(mk("big256-nt", ("big", 256, "0", "tr"), Mb, 256, 128, tb=True))
    out.append(mk("big256-nn-ldd259", ("big", 256, "0", "rows"), Mb, 256, 128, ldd=259, bias=True))
    out.append(mk("big320-nt", ("big", 320, "0", "rows"), Mb, 320, 128, tb=True, bias=True))
    out.append(mk("big256-nt-tanh_out", ("big", 256, "E_DACT", "tr"), Mb, 256, 128, tb=True, dact=ACT_TANH_OUT))
    out.append(mk("big320-nt-tanh_out", ("big", 320, "E_DACT", "rows"), Mb, 320, 128, tb=True, dact=ACT_TANH_OUT, bias=True))
    # ---- generic bf16: one case per refusal rule of tfasr_gemm_fast_try, the four layouts, full epilogue chains
    GB = ("generic", "bf16", 128)
    lin = dict(bias=True, prez=True, dact=ACT_FACTOR, drop_p=0.5, res=True)
    non = dict(bias=True, prez=True, act=ACT_SWISH, dact=ACT_TANH, drop_p=0.75, res=True)
    out.append(mk("gbf-a-off-16-bytes-nn", GB, 200, 144, 136, a_off=1, **lin))
    out.append(mk("gbf-b-off-16-bytes-nt", GB, 200, 144, 136, tb=True, b_off=1, **non))
    out.append(mk("gbf-lda-203-tn", GB, 200, 144, 136, ta=True, lda=203, **lin))
    out.append(mk("gbf-ldb-139-tt", GB, 200, 144, 136, ta=True, tb=True, ldb=139, **non))
    out.append(mk("gbf-k5-nn", GB, 200, 144, 5, lda=8, **lin))
    out.append(mk("gbf-n36-ldb36-nn", GB, 130, 36, 72, ldb=36, **non))
    out.append(mk("gbf-m36-lda36-tn", GB, 36, 144, 72, ta=True, lda=36, **lin))
    out.append(mk("gbf-m36-lda36-tt-f32out", GB, 36, 144, 72, ta=True, tb=True, lda=36, out_f32=True, bias=True, res=True))
    # ---- generic f32: 64-wide below 2 CUs tiles (N > 64), else 128-wide
    for ln, ta, tb in LAYOUTS:
        e = lin if ln in ("nn", "tt") else non
        out.append(mk(f"gf32-200x144x20-{ln}", ("generic", "f32", 64), 200, 144, 20, ta=ta, tb=tb, dtype="f32", **e))
        out.append(mk(f"gf32-77x40x19-{ln}", ("generic", "f32", 128), 77, 40, 19, ta=ta, tb=tb, dtype="f32", **e))
    out.append(mk("gf32-wide-n384", ("generic", "f32", 128), Mo, 384, 20, dtype="f32", bias=True))
    out.append(mk("gf32-wide-n384-first-300-rows", ("generic", "f32", 64), 300, 384, 20, dtype="f32", bias=True))
    # ---- output addressing on persist64, one64 and persist128: padded rows (ldd = N + 8), odd rows (N + 3: the element-wise stores and
    # the per-element dropout hash), batches at an odd offset, D off 16 bytes; D, res, dact_z and prez all follow ldd
    Mq = 128 * ceil_div(2 * cus + 1, 3 * 6) - 37   # one64 with 2 x 3 batches: more than 2 CUs 64-wide tiles in all
    Mr = 128 * (cus // 18 + 1) - 37                # persist128 with 2 x 3 batches: more than CUs 128-wide tiles in all
    for pre, lab, M, N, K, Mbat in (("p64c", P64, Mp, 192, 136, 219), ("o64", O64, Mo, 192, 136, Mq), ("p128", P128, M1, 384, 320, Mr)):
        for pad in (8, 3):
            _compiled(f"{pre}-ldd+{pad}", lab, M, N, K, out, which=("res_drop", "act_drop", "dact_drop"), ldd=N + pad, kinds=("exact",))
        _compiled(f"{pre}-d-off-2-bytes", lab, M, N, K, out, which=("res_drop", "act_drop", "dact_drop"), d_off=1, kinds=("exact",))
        bl = lab if pre != "p64c" else P64  # (the small batched product: E_RES | E_DROP is compiled at every size, the swish' one is not)
        _compiled(f"{pre}-batched", bl, Mbat, N, K, out, which=("res_drop",), nb1=2, nb2=3, kinds=("exact",))
        if pre == "p64c":
            out.append(mk("p64c-batched-dact_drop", P64 + ("E_GEN",), Mbat, N, K, tb=True, dact=ACT_SWISH, drop_p=0.5, nb1=2, nb2=3, kinds=("exact",)))
        else:
            _compiled(f"{pre}-batched", bl, Mbat, N, K, out, which=("dact_drop",), nb1=2, nb2=3, kinds=("exact",))
    table = {c.name: c for c in out}
    assert len(table) == len(out), "case names must be unique"
    return table


def group_cases():
    """tfasr_gemm_group: the weight gradients of test_grouped_weight_gradients_one_launch with K cut to 1000 / 993 / 150"""
    return [mk(f"group-{i}-{M}x{N}x{K}", ("group", 128, "E_CSUM"), M, N, K, ta=True, accumulate=True, out_f32=True, colsum=cs)
            for i, (M, N, K, cs) in enumerate(GROUP_SHAPES)]


ROUTES = [  # every label of the issue's route list: each must be the label of at least one exact and one random case
    ("fast", 64, "persist", "0"), ("fast", 64, "persist", "E_RES"), ("fast", 64, "persist", "E_RES|E_DROP"), ("fast", 64, "persist", "E_GEN"),
    ("fast", 64, "persist", "E_ACT"), ("fast", 64, "persist", "E_ACT|E_DROP"), ("fast", 64, "persist", "E_DACT"),
    ("fast", 64, "persist", "E_DACT|E_DROP"), ("fast", 64, "persist", "E_MUL"), ("fast", 64, "persist", "E_CSUM"),
    ("fast", 64, "one", "0"), ("fast", 64, "one", "E_RES"), ("fast", 64, "one", "E_RES|E_DROP"), ("fast", 64, "one", "E_ACT"),
    ("fast", 64, "one", "E_ACT|E_DROP"), ("fast", 64, "one", "E_DACT"), ("fast", 64, "one", "E_DACT|E_DROP"), ("fast", 64, "one", "E_MUL"),
    ("fast", 64, "one", "E_GEN"),
    ("fast", 128, "persist", "0"), ("fast", 128, "persist", "E_RES"), ("fast", 128, "persist", "E_RES|E_DROP"), ("fast", 128, "persist", "E_ACT"),
    ("fast", 128, "persist", "E_ACT|E_DROP"), ("fast", 128, "persist", "E_DACT"), ("fast", 128, "persist", "E_DACT|E_DROP"),
    ("fast", 128, "persist", "E_MUL"), ("fast", 128, "persist", "E_GEN"), ("fast", 128, "persist", "E_CSUM"),
    ("big", 256, "0", "tr"), ("big", 256, "0", "rows"), ("big", 320, "0", "rows"), ("big", 256, "E_DACT", "tr"), ("big", 320, "E_DACT", "rows"),
    ("generic", "bf16", 128), ("generic", "f32", 64), ("generic", "f32", 128), ("generic+colsum", "bf16", 128), ("generic+colsum", "f32", 64),
]
