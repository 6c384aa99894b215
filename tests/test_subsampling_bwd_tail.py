"""CPU: the subsampling backward over folded padded tails (DESIGN.md section 2 "Padded tail"), float64 and host geometry only.

  * the identity: with the gradient w.r.t. conv2's output replaced, per utterance, by its sum over the tail in row r (and zero behind),
    conv2's weight / bias gradient and the sums of the one-pass conv1 + BatchNorm0 backward (bstats, P, sum dz) are what the unfolded
    gradient gives, given a feature map that is constant in time behind each utterance's first constant frame; a bf16 hi / lo pair
    leaves a residue below 2^-17 of the sum, which moves conv2's weight gradient by no more than 2^-17 of its sum of |terms| - the
    GPU route keeps a third term (2^-25), since 2^-17 of a like-signed tail is above the f32 summation error of the full route;
  * the host tables of ConformerTransducer._tail_bwd_geometry against a brute-force enumeration (the batch of the GPU test and B = 1), and
    the rows tfasr_s2d_tail_fold clears against every row a computed block can read."""
import numpy as np
import pytest
import torch

import subsampling_oracle as so
from tensorflowasr_amd.conformer import ConformerTransducer as CT

T0 = 400
TF = [401, 150, 199, 30, 396]  # first constant feature frame per utterance (tests/test_subsampling_padded_tail_gpu.py)


# ------------------------------------------------------------------------------------------------------------------ the identity
def constant_tail_case(F0=10, C=8, seed=3):
    g = torch.Generator().manual_seed(seed)
    B = len(TF)
    x = so.logmel_like(g, (B, T0, F0), torch.float64)
    for b, t in enumerate(TF):
        if t < T0:
            x[b, t:] = x[b, t].clone()
    w0, b0 = torch.randn(3, 3, 1, C, generator=g, dtype=torch.float64) * 0.3, torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    gamma, beta = 1.0 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64), 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    T1, F1, T2, F2 = so.dims(T0, F0)
    z, _ = so.conv1(x, w0, b0)
    fin = so.finalize(so.stats(z)["stats"], B * T1 * F1, gamma, beta)
    a1 = so.bn0_apply(x, w0, b0, fin)["y"]
    W = torch.randn(9 * C, C, generator=g, dtype=torch.float64) * 0.1
    bias = torch.randn(C, generator=g, dtype=torch.float64) * 0.1
    do = torch.randn(B, T2, F2, C, generator=g, dtype=torch.float64) + 0.3  # like-signed on average: the sums grow with the tail
    return dict(x=x, w0=w0, b0=b0, fin=fin, a1=a1, W=W, bias=bias, do=do, dims=(B, T1, F1, T2, F2, C))


def backward(c, do):
    """every gradient downstream of `do` (dense [B, T2, F2, C], time row tt = index + 1)"""
    B, T1, F1, T2, F2, C = c["dims"]
    g2 = so.conv2(c["a1"], c["W"], c["bias"], do)
    g1 = so.bn0_backward(c["x"], c["w0"], c["b0"], c["fin"], g2["dx"], B * T1 * F1)
    scale = dict(dw=g1["M_dw_onepass"], db=g1["M_db_onepass"])  # conv1's bias gradient is zero analytically: judged on its terms
    return dict(gW=g2["dW"], gb=g2["db"], bstats=g1["bstats"], P=g1["P"], dw=g1["dw_onepass"], db=g1["db_onepass"]), scale


def fold(do, r, T2, terms):
    """the replacement tfasr_s2d_tail_fold makes, in float64; the sum as `terms` bf16 rows (the kernel: 3), terms = 0: whole in row r"""
    out = do.clone()
    for b, rb in enumerate(r):
        if rb + 3 > T2:
            continue
        S = do[b, rb - 1:].sum(0)
        out[b, rb - 1:] = 0
        if terms == 0:
            out[b, rb - 1] = S
        for k in range(terms):
            out[b, rb - 1 + k] = S.float().bfloat16().double()
            S = S - out[b, rb - 1 + k]
    return out


def test_fold_then_backward_equals_backward():
    c = constant_tail_case()
    B, T1, F1, T2, F2, C = c["dims"]
    r = [int(v) for v in CT._tail_rows(np.array(TF), T0)["o"]]
    assert [rb + 3 <= T2 for rb in r] == [False, True, True, True, False]  # no tail, three folded, a tail shorter than the margins
    # premise: a1 is constant from S row r - 1 on, i.e. conv1 rows >= 2 (r - 1) - 2
    for b, rb in enumerate(r):
        if rb + 3 <= T2:
            t1 = 2 * (rb - 1) - 2
            assert torch.equal(c["a1"][b, t1:], c["a1"][b, t1:t1 + 1].expand(T1 - t1, -1, -1)), b
    ref, scale = backward(c, c["do"])
    got, _ = backward(c, fold(c["do"], r, T2, 0))
    for k in ref:
        err, of = float((got[k] - ref[k]).abs().max()), float(scale.get(k, ref[k]).abs().max())
        print(k, "max |fold - full|", err, "of", of)
        assert err <= 1e-10 * of, k
    assert not torch.equal(fold(c["do"], r, T2, 0), c["do"])


@pytest.mark.parametrize("terms,eps", [(2, 2.0 ** -17), (3, 2.0 ** -25)])
def test_bf16_terms_keep_the_sum(terms, eps):
    c = constant_tail_case()
    B, T1, F1, T2, F2, C = c["dims"]
    r = [int(v) for v in CT._tail_rows(np.array(TF), T0)["o"]]
    pair = fold(c["do"], r, T2, terms)
    absS = torch.zeros_like(c["do"])
    for b, rb in enumerate(r):
        if rb + 3 <= T2:
            S = c["do"][b, rb - 1:].sum(0)
            assert bool(((pair[b, rb - 1:rb - 1 + terms].sum(0) - S).abs() <= eps * S.abs()).all())
            assert bool((pair[b, rb - 1 + terms:] == 0).all())
            # one bf16 row alone would not do: 2^-9 of sums of dozens of terms
            assert float((pair[b, rb - 1] - S).abs().max()) > 2.0 ** -12 * float(S.abs().max())
            absS[b, rb - 1] = S.abs()
    ref, got = backward(c, c["do"])[0], backward(c, pair)[0]
    bound = so.conv2(c["a1"].abs(), c["W"], c["bias"], absS)
    assert bool(((got["gW"] - ref["gW"]).abs() <= eps * bound["dW"] + 1e-12).all())
    assert bool(((got["gb"] - ref["gb"]).abs() <= eps * bound["db"] + 1e-12).all())
    # the sums behind the data gradient: the residue through |W| and the sums of |terms| of the BatchNorm0 backward
    da1 = so.conv2(c["a1"], c["W"].abs(), c["bias"], absS)["dx"]
    m = so.bn0_backward(c["x"], c["w0"], c["b0"], c["fin"], da1, B * T1 * F1)
    assert bool(((got["bstats"] - ref["bstats"]).abs() <= eps * m["M_bstats"] + 1e-12).all())
    assert bool(((got["P"] - ref["P"]).abs() <= eps * m["M_P"] + 1e-12).all())


# --------------------------------------------------------------------------------------------------------------- the host tables
def brute(tf, B, T2, F2, T1):
    r = CT._tail_rows(np.array(tf), T0)["o"]
    rows = B * (T2 + 1) * (F2 + 1)
    real = np.zeros(rows, bool)
    listed = []
    for b in range(B):
        folded = r[b] + 3 <= T2
        for tt in range(1, T2 + 1):
            if not folded or tt < r[b] + 3:
                real[(b * (T2 + 1) + tt) * (F2 + 1):(b * (T2 + 1) + tt + 1) * (F2 + 1)] = True
        listed += [b * T1 + t for t in range(T1) if not folded or t < 2 * (r[b] + 2)]
    nblk = -(-rows // 256)
    comp = [k for k in range(nblk) if real[k * 256:(k + 1) * 256].any()]
    return comp, [k for k in range(nblk) if k not in comp], [int(r[b]) if r[b] + 3 <= T2 else T2 + 1 for b in range(B)], listed, real


@pytest.mark.parametrize("tf", [TF, [150], [401], [30, 30, 30]])
def test_tables_against_enumeration(tf):
    B, T1, T2, F2 = len(tf), 200, 100, 20
    comp, skip, r, rows = CT._tail_bwd_geometry(np.array(tf), B, T0, T2, F2)
    bc, bs, br, bl, real = brute(tf, B, T2, F2, T1)
    assert list(comp) == bc and list(skip) == bs and list(r) == br and list(rows) == bl
    assert list(comp) == sorted(comp)  # the K-block table must be ascending
    # every row a computed block can read (its own 256 and F2 + 2 either side) is real, a hi / lo row, or a row the fold clears
    zr = (255 + F2 + 2 + F2) // (F2 + 1) + 1  # csrc/conv2d.hip tfasr_s2d_tail_fold
    slack, total = F2 + 2, B * (T2 + 1) * (F2 + 1)
    for k in comp:
        for row in range(max(0, k * 256 - slack), min(total, (k + 1) * 256 + slack)):
            b, tt = row // ((T2 + 1) * (F2 + 1)), row // (F2 + 1) % (T2 + 1)
            if real[row] or tt == 0:  # (halo rows are zeroed by tfasr_halo_zero)
                continue
            assert tt >= r[b] + 3 and (tt < r[b] + 3 + zr or tt > T2 - zr), (k, row, b, tt)


def test_backward_skips_fewer_blocks_than_the_forward():
    comp, skip, _ = CT._tail_blocks(np.array(TF), 5, T0, 100, 20)
    bcomp, bskip, r, rows = CT._tail_bwd_geometry(np.array(TF), 5, T0, 100, 20)
    assert set(comp) <= set(bcomp) and 0 < len(bskip) <= len(skip)
    assert len(rows) < 5 * 200
