"""The fused relative-position attention of csrc/attn_fused.hip, forward and backward, restated plainly in float64 torch on the CPU: closed
form on the T x T score matrix, no autograd inside.  tests/test_relattn_fused_gpu.py holds every kernel of that file to these functions on
every launch branch; tests/test_relattn_oracle.py pins them against torch autograd on oracle/conformer_ref.py::rel_attention_core (the
reference's own formulation: rel_left_shift, the rolled / zeroed position encoding, compute_streaming_mask, the auto mask) and shows that
the bounds below admit a kernel with the rounding points of the real one and reject seven subtly wrong ones.

Follows  MultiHeadRelativeAttention._compute_attention    multihead_attention.py:543-582, relative shift :27-77, streaming mask :104-143
         RelativeSinusoidalPositionalEncoding.call          positional_encoding.py:152-172 (per-sample roll, zero past 2 len - 1)

    s_ij   = scale [ (q_i + u) . k_j + (q_i + v) . pext[idx(i, j)] ]
    idx    = r + T - len  if  r = T - 1 - i + j < 2 len - 1   else  the bias row 2T - 1
    window = keys [lo, hi) of stream_window (attn_fused.hip:144-148): lo = max(0, (i / chunk) chunk - hist) (0 for hist < 0),
             hi = min(T, (i / chunk) chunk + chunk); outside it the probability is exactly 0
    mask   = padded QUERY rows (i >= len) have constant scores over ALL T keys: out = mean_j v_j, lse = log T; keys are never masked
The functions take the values the kernels are given (bf16 qkv [B*T, 3*H*64], f32 u / v, bf16 pext [2T, H*64], lengths, scale, use_mask,
chunk, hist) and return dicts of float64 tensors in the kernels' layouts.  The one rounding point that is bit-defined is taken as the kernel
takes it (q_frag, :108-115): qu = bf16(q + u), qv = bf16(q + v), f32 add then round to nearest even.  Under "M_<name>" the magnitude sums:
    M_out = sum_j p_ij |v_j|          M_s = sum |qu||k| + sum |qv||pext[idx]|          M_dS = p (sum |dO||v| + sum |dO||o|) scale
    M_dq, M_dk, M_dv, M_du, M_dvb, M_dpext: the gradient's own sum over M_dS (or p) and the absolute second factor

THE BOUNDS, with U16 = 2^-8 (bf16 unit roundoff), U32 = 2^-24, E = ELEM_RTOL = 1e-5 and ELEM_ATOL = 1e-6 (the suite's element bound of
tests/gemm_oracle.py / test_pointwise_gpu._elem_bound for one fast transcendental: v_exp_f32 and v_log_f32 are 1-ulp instructions, 2^-23
relative, so that bound applies to them with room).  No constant below was fitted to what a GPU returned.
 score    :313 / :324 / :707 / :720 / :1224 / :1239 accumulate 64 + 64 bf16 products in f32, :349 / :355 add the two parts, :386 / :758 /
          :780 / :1289 form the exponent with one more product and a fused multiply-add against m (or lse):
              e_s = (128 + 2) U32 scale M_s + 4 U32 |s|            and per row  eps_i = max_j e_s + E  (exp2, relative, on every p_ij)
 out      :395 rounds P to bf16 for P V while :394 sums the UNROUNDED f32 values into l: U16 M_out.  P V (:415) and l (:394-401) are f32
          sums of T terms, rescaled once per key block (:401 / :404; the factor is common to both, its rounding is not): (T + 2 + 2 nblk) U32
          each.  A relative perturbation eps of every p_ij moves the normalised sum by at most expm1(2 eps) M_out.  :432 stores bf16:
              B_out = X + U16 (|out| + X),    X = [U16 + expm1(2 eps_i) + 2 (T + 2 + 2 nblk) U32] M_out
 lse      :436 m ln 2 + logf(l); l carries eps_i and its f32 sum; logf the element bound; two f32 operations on |m| and |log l|:
              B_lse = eps_i + (T + 2 + 2 nblk) U32 + E |log l| + ELEM_ATOL + 4 U32 (|m| + |log l|)
 D, bias  :482 / :494 f32 sums of 64 products, reduced over four lanes: (64 + 2) U32 sum |dO||o|,  (64 + 2) U32 sum |qv||pext[R]|
 dS       :760 / :782 (query side) and :1291 (key side) form p (dP - D) scale in f32 - p with e_s + 2 U32 |lse| + E, dP (:708 / :1225) and D
          with (64 + 2) U32 of their terms, three more f32 operations - and :761 / :785 / :1071 round it to bf16 for the products (the
          bias-row share :783 is summed unrounded, which only helps):
              kappa = max (e_s + 2 U32 |lse|) + E + 70 U32,        B_dS = U16 |dS| + (1 + U16) kappa M_dS
 P^T      :1071 (img_store) rounds p to bf16 for dv = P^T dO: U16 and kappa on M_dv
 dq dk dv :821 / :829 / :1309 / :1310 f32 sums over the T keys (queries) - dq over keys and over window columns: 2T - and :861 / :1335 a bf16 store:
              B_g = X + U16 (|g| + X),        X = [U16 + (1 + U16) kappa + (n + 4) U32] M_g,      n = 2T for dq, T for dk and dv
 du dvb   :876-892 column sums of the f32 dq_u / dq_v over the rows of a block, then f32 atomics over the blocks: no store rounding,
              B = [U16 + (1 + U16) kappa + (B T + T + 4) U32] M
 dpext    :1014 f32 sums of dS (as stored: bf16) times qv over the queries and samples of a group, :1032 one f32 atomic per group: from given
          dS and qv (B T + 2) U32 M_dpext, f32 accumulation only; chained, the rows carry B_dS: the du coefficient.  The bias row (:883-892)
          sums the unrounded f32 dS: the same without the U16 term.
 chained  (backward from the GPU's own o and lse against the oracle's exact ones) p carries B_lse as well and D the error of o: with
          c_out = max B_out / M_out and M_dS taken over M_out in place of |o| (`o_mag`), kappa grows by max B_lse + c_out.
"""
import math
from collections import namedtuple

import torch

from gemm_oracle import ELEM_ATOL, ELEM_RTOL

DH = 64
U16 = 2.0 ** -8
U32 = 2.0 ** -24
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64

Case = namedtuple("Case", "B H T lens use_mask chunk hist dhl amp")
# id -> shape, lengths, mask / window (chunk 0: no window; hist -1: unlimited history), logical head size, input amplitude.  `amp` is the
# standard deviation of q, k, v and the table (u / v: 0.3, dout: 1): 0.7, the scale of the attention tests of test_ops_gpu.py, at which the
# reference alone decides every mutant (test_relattn_oracle.py); 1.5 where the forward bound is probed nearer its edge.
CASES = {
    "t1": Case(3, 4, 1, (1, 1, 1), True, 0, 0, 64, 0.7),
    "t9": Case(3, 3, 9, (9, 5, 1), True, 0, 0, 64, 0.7),
    "t63": Case(2, 4, 63, (63, 17), True, 0, 0, 64, 0.7),
    "t64": Case(2, 4, 64, (64, 1), True, 0, 0, 64, 0.7),
    "t65": Case(2, 4, 65, (65, 64), True, 0, 0, 64, 1.5),
    "h1": Case(1, 1, 130, (130,), True, 0, 0, 64, 0.7),
    "h8": Case(2, 8, 130, (130, 97), True, 0, 0, 64, 0.7),
    "pad-block": Case(4, 4, 200, (200, 128, 65, 1), True, 0, 0, 64, 0.7),
    "nomask": Case(2, 4, 130, (130, 60), False, 0, 0, 64, 0.7),
    "heads36": Case(3, 4, 150, (150, 70, 1), True, 0, 0, 36, 0.7),
    "win-16-64": Case(3, 4, 150, (150, 70, 1), True, 16, 64, 64, 0.7),
    "win-5-3": Case(2, 4, 150, (150, 99), True, 5, 3, 64, 0.7),
    "win-1-0": Case(2, 4, 70, (70, 33), True, 1, 0, 64, 1.5),
    "win-8-inf": Case(2, 4, 130, (130, 64), True, 8, -1, 64, 0.7),
    "win-wide": Case(2, 4, 70, (70, 20), True, 80, 0, 64, 0.7),
    "dpext-groups": Case(11, 32, 130, (130, 1, 2, 97, 40, 63, 130, 17, 64, 129, 5), True, 0, 0, 64, 0.7),
}


def dpext_bchunk(B, H, T):
    """samples per workgroup group of tfasr_relattn_dpext (attn_fused.hip:1469-1475)"""
    cblocks = (2 * T - 1 + 127) // 128
    groups = max(1, min(B, 1024 // max(1, cblocks * H)))
    return -(-B // groups)


def make_inputs(name):
    """The case's inputs as the kernels take them (CPU tensors): bf16 qkv / pext / dout, f32 u / v; dims dhl..63 of every head zero."""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    HD = c.H * DH
    keep = (torch.arange(DH) < c.dhl).repeat(c.H)
    qkv = (torch.randn(c.B * c.T, 3 * HD, generator=g) * c.amp * keep.repeat(3)).to(BF)
    u, v = torch.randn(HD, generator=g) * 0.3 * keep, torch.randn(HD, generator=g) * 0.3 * keep
    pext = (torch.randn(2 * c.T, HD, generator=g) * c.amp * keep).to(BF)
    dout = (torch.randn(c.B * c.T, HD, generator=g) * keep).to(BF)
    return dict(qkv=qkv, u=u, v=v, pext=pext, dout=dout, lens=list(c.lens), B=c.B, H=c.H, T=c.T, scale=1.0 / math.sqrt(c.dhl),
                use_mask=c.use_mask, chunk=c.chunk, hist=c.hist)


# ------------------------------------------------------------------------------------ index arithmetic
def pair_index(T, lens):
    """idx [B, T, T]: the table row of pair (i, j)"""
    ln = torch.tensor(lens).clamp(max=T)[:, None, None]
    r = (T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :])[None]
    return torch.where(r < 2 * ln - 1, r + T - ln, torch.full_like(r, 2 * T - 1))


def padded_rows(T, lens, use_mask):
    """[B, T] bool: query rows with constant scores"""
    ln = torch.tensor(lens).clamp(max=T)[:, None]
    return (torch.arange(T)[None] >= ln) & bool(use_mask)


def window(T, chunk, hist):
    """lo, hi [T] of stream_window; chunk <= 0: the whole utterance"""
    i = torch.arange(T)
    if chunk <= 0:
        return torch.zeros_like(i), torch.full_like(i, T)
    index = (i // chunk) * chunk
    lo = torch.zeros_like(i) if hist < 0 else (index - hist).clamp(min=0)
    return lo, (index + chunk).clamp(max=T)


def visible(T, lo, hi, padded):
    """[B, T, T] bool: keys a query row sums over (a padded row: all of them)"""
    j = torch.arange(T)[None, :]
    return ((j >= lo[:, None]) & (j < hi[:, None]))[None] | padded[:, :, None]


def live_rows(T, lens, use_mask):
    """[B, T] bool: rows of the 64-query blocks that are not wholly padding - the rows whose qu / qv / dvec / dS are written"""
    live = torch.ones(len(lens), T, dtype=torch.bool)
    if use_mask:
        for b, n in enumerate(lens):
            live[b, min(-(-min(n, T) // 64) * 64, T):] = False
    return live


def _rows(x):  # [B, H, T, DH] -> [B*T, H*DH]
    B, H, T, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * T, H * D)


def _heads(x, B, H, T):  # [B*T, H*DH] -> [B, H, T, DH] float64
    return torch.as_tensor(x).detach().cpu().to(F64).view(B, T, H, DH).permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------ forward
def forward(qkv, u, v, pext, lens, B, H, T, scale, use_mask=True, chunk=0, hist=0, idx=None, vis=None, padded=None):
    """-> out [B*T, H*64], lse [B, H, T], qu, qv [B*T, H*64] and their magnitudes; the private entries (leading underscore) are what
    backward() continues from.  idx / vis / padded: the index arithmetic, if the caller has its own (the mutants of test_relattn_oracle.py)."""
    x = qkv.detach().cpu().to(F32).view(B, T, 3, H, DH)
    qu = (x[:, :, 0] + u.detach().cpu().to(F32).view(H, DH)).to(BF).to(F64).permute(0, 2, 1, 3)
    qv = (x[:, :, 0] + v.detach().cpu().to(F32).view(H, DH)).to(BF).to(F64).permute(0, 2, 1, 3)
    k, vv = x[:, :, 1].to(F64).permute(0, 2, 1, 3), x[:, :, 2].to(F64).permute(0, 2, 1, 3)
    pe = pext.detach().cpu().to(F64).view(2 * T, H, DH).permute(1, 0, 2)  # [H, 2T, DH]
    idx = pair_index(T, lens) if idx is None else idx
    padded = padded_rows(T, lens, use_mask) if padded is None else padded
    vis = visible(T, *window(T, chunk, hist), padded) if vis is None else vis
    idxe = idx[:, None].expand(B, H, T, T)
    pm = padded[:, None, :, None]
    s = (qu @ k.transpose(2, 3) + torch.gather(torch.einsum("bhid,hcd->bhic", qv, pe), 3, idxe)) * scale
    M_s = qu.abs() @ k.abs().transpose(2, 3) + torch.gather(torch.einsum("bhid,hcd->bhic", qv.abs(), pe.abs()), 3, idxe)
    s, M_s = s.masked_fill(pm, 0.0), M_s.masked_fill(pm, 0.0)
    sm = s.masked_fill(~vis[:, None], -math.inf)
    lse = torch.logsumexp(sm, -1)
    p = torch.exp(sm - lse[..., None])
    return dict(out=_rows(p @ vv), lse=lse, qu=_rows(qu), qv=_rows(qv), M_out=_rows(p @ vv.abs()), M_s=M_s,
                _p=p, _s=s, _sm=sm, _qu=qu, _qv=qv, _k=k, _v=vv, _pe=pe, _idx=idx, _vis=vis, _padded=padded,
                B=B, H=H, T=T, scale=scale)


def forward_bounds(f):
    """B_out [B*T, H*64], B_lse [B, H, T] (module docstring)"""
    T, scale = f["T"], f["scale"]
    acc = (T + 2 + 2 * -(-T // 64)) * U32
    vis = f["_vis"][:, None]
    e_s = (130 * U32 * scale * f["M_s"] + 4 * U32 * f["_s"].abs()).masked_fill(~vis, 0.0)
    eps = e_s.amax(-1) + ELEM_RTOL
    X = (U16 + torch.expm1(2 * eps) + 2 * acc)[..., None].expand(-1, -1, -1, DH)
    X = _rows(X.contiguous()) * f["M_out"]
    m = f["_sm"].amax(-1)
    logl = (f["lse"] - m).abs()
    return dict(out=X + U16 * (f["out"].abs() + X), lse=eps + acc + ELEM_RTOL * logl + ELEM_ATOL + 4 * U32 * (m.abs() + logl), e_s=e_s)


# ------------------------------------------------------------------------------------ backward
def _scatter(f, w):
    """[B, H, T, T] over (i, j) -> [B, H, T, 2T] over (i, table row)"""
    B, H, T = f["B"], f["H"], f["T"]
    return torch.zeros(B, H, T, 2 * T, dtype=F64).scatter_add_(3, f["_idx"][:, None].expand(B, H, T, T), w)


def backward(f, o, lse, dout, o_mag=None):
    """From the forward's inputs (f = forward(...)) and the GIVEN o [B*T, H*64], lse [B, H, T], dout: p = exp(s - lse) on the visible keys,
    D_i = rowsum(dout o), dS = p (dP - D) scale (0 at padded rows) -> dvec [2, B, H, T] (D | the bias-row score), dS [B, H, T, T] unskewed
    and zero at the bias-row pairs, dq = dqu + dqv, dk, dv [B*T, H*64], du, dvb [H*64], dpext [2T, H*64] (bias row included).
    o_mag: what stands for |o| in M_dS (the chained bound: M_out)."""
    B, H, T, scale = f["B"], f["H"], f["T"], f["scale"]
    qu, qv, k, vv, pe = f["_qu"], f["_qv"], f["_k"], f["_v"], f["_pe"]
    o, do = _heads(o, B, H, T), _heads(dout, B, H, T)
    om = o.abs() if o_mag is None else _heads(o_mag, B, H, T)
    lse = torch.as_tensor(lse).detach().cpu().to(F64)
    p = torch.exp(f["_sm"] - lse[..., None])
    real = ~f["_padded"][:, None, :, None]
    D = (do * o).sum(-1)
    dS = p * (do @ vv.transpose(2, 3) - D[..., None]) * scale * real
    M_dS = p * (do.abs() @ vv.abs().transpose(2, 3) + (do.abs() * om).sum(-1)[..., None]) * scale * real
    table = (f["_idx"] != 2 * T - 1)[:, None]
    G, MG = _scatter(f, dS), _scatter(f, M_dS)
    dqu, dqv = dS @ k, torch.einsum("bhic,hcd->bhid", G, pe)
    M_dqu, M_dqv = M_dS @ k.abs(), torch.einsum("bhic,hcd->bhid", MG, pe.abs())
    r = dict(dvec=torch.stack([D, torch.einsum("bhid,hd->bhi", qv, pe[:, 2 * T - 1])]),
             M_dvec=torch.stack([(do.abs() * o.abs()).sum(-1), torch.einsum("bhid,hd->bhi", qv.abs(), pe[:, 2 * T - 1].abs())]),
             dS=dS * table, M_dS=M_dS, dq=_rows(dqu + dqv), M_dq=_rows(M_dqu + M_dqv),
             dk=_rows(dS.transpose(2, 3) @ qu), M_dk=_rows(M_dS.transpose(2, 3) @ qu.abs()),
             dv=_rows(p.transpose(2, 3) @ do), M_dv=_rows(p.transpose(2, 3) @ do.abs()),
             du=dqu.sum((0, 2)).reshape(-1), M_du=M_dqu.sum((0, 2)).reshape(-1), dvb=dqv.sum((0, 2)).reshape(-1), M_dvb=M_dqv.sum((0, 2)).reshape(-1),
             dpext=torch.einsum("bhic,bhid->chd", G, qv).reshape(2 * T, H * DH), M_dpext=torch.einsum("bhic,bhid->chd", MG, qv.abs()).reshape(2 * T, H * DH),
             _lse=lse)
    return r


def dpext_of(f, ds):
    """The table gradient tfasr_relattn_dpext forms from a GIVEN unskewed dS [B, H, T, >= T] (as stored: bf16, zero at the bias-row pairs)
    and the oracle's qv: rows 0 .. 2T-2; the bias row is not its to write."""
    T, H = f["T"], f["H"]
    ds = torch.as_tensor(ds).detach().cpu().to(F64)[..., :T] * (f["_idx"] != 2 * T - 1)[:, None]
    d = torch.einsum("bhic,bhid->chd", _scatter(f, ds), f["_qv"]).reshape(2 * T, H * DH)
    M = torch.einsum("bhic,bhid->chd", _scatter(f, ds.abs()), f["_qv"].abs()).reshape(2 * T, H * DH)
    d[2 * T - 1], M[2 * T - 1] = 0.0, 0.0
    return dict(dpext=d, M_dpext=M, B_dpext=(f["B"] * T + 2) * U32 * M)


def backward_bounds(f, fb, bk, chained=False):
    """Bounds of every entry of bk = backward(f, ...) (module docstring); fb = forward_bounds(f).  chained: bk was formed with
    o_mag = f["M_out"] from the oracle's exact o and lse, and the kernels ran from the GPU's."""
    B, T = f["B"], f["T"]
    kappa = float((fb["e_s"] + 2 * U32 * bk["_lse"].abs()[..., None]).max()) + ELEM_RTOL + 70 * U32
    if chained:
        ok = f["M_out"] > 0
        kappa += float(fb["lse"].max()) + (float((fb["out"][ok] / f["M_out"][ok]).max()) if bool(ok.any()) else 0.0)
    c = (1 + U16) * kappa

    def stored(g, M, n):
        X = (U16 + c + (n + 4) * U32) * M
        return X + U16 * (g.abs() + X)

    csum = U16 + c + (B * T + T + 4) * U32
    rows = torch.full((2 * T, 1), csum, dtype=F64)
    rows[2 * T - 1] = csum - U16
    return dict(dvec=66 * U32 * bk["M_dvec"], dS=U16 * bk["dS"].abs() + c * bk["M_dS"], dq=stored(bk["dq"], bk["M_dq"], 2 * T),
                dk=stored(bk["dk"], bk["M_dk"], T), dv=stored(bk["dv"], bk["M_dv"], T), du=csum * bk["M_du"], dvb=csum * bk["M_dvb"],
                dpext=rows * bk["M_dpext"], kappa=kappa)
