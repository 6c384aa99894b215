"""GPU: the subsampling backward over folded padded tails (ConformerTransducer._sub_tail_bwd; DESIGN.md section 2 "Padded tail").

tfasr_s2d_tail_fold replaces each utterance's tail of the gradient w.r.t. conv2's output by its sum over time (three bf16 terms in three rows);
the conv2 weight gradient then runs over the 256-row blocks of K that are left (tfasr_gemm_args.k_tiles), the data gradient over the same
blocks of its output (row_tiles) and the one-pass conv1 + BatchNorm0 backward over a list of conv1 rows.  Checked here:
  * the fold kernel against numpy float64: the sum of the three rows, rows in front bitwise, the zeros a computed block can reach, halo columns;
  * the K-block table, single launch and grouped, with column sums: NaN in every unlisted block of both operands, the result finite and
    the float64 product over the listed rows (bounds of test_gemm_gpu.py's split-K weight gradients); validation;
  * the row list of the one-pass backward: NaN in the gradient at unlisted rows against the full call on a gradient zeroed there, both
    within the float64 bounds of test_conv2d_gpu.py;
  * the model, switch on against off, one backward from the same gradient: what is computed before the fold bitwise equal, every
    gradient behind it no further from float64 than twice what the full route is;
  * the f32 model, `sub_norm="layer"`, `_conv1_gram` off and a feature map that is not the front end's take the full route.
Batch of the model tests: that of test_subsampling_padded_tail_gpu.py (B = 5, 400 frames, C = 64)."""
import ctypes

import numpy as np
import pytest
import torch

import subsampling_oracle as so
from tensorflowasr_amd import _lib, configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
STEP = 160
T0 = 400
TF = [401, 150, 199, 30, 396]
NSAMP = [T0 * STEP] + [t * STEP - 1 for t in TF[1:]]
NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------ the fold kernel
def test_fold_kernel_against_float64(dev):
    B, T2, F2, C = 3, 30, 6, 16
    r = [4, 9, 29]  # 29 + 3 > T2: left alone
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, T2 + 1, F2 + 1, C, generator=g) + 0.4).to(BF16)
    x[:, 0] = 0
    x[:, :, 0] = 0
    xd = x.to(dev)
    scratch = torch.zeros(B, F2 + 1, C, device=dev)
    K.s2d_tail_fold(xd, torch.tensor(r, dtype=torch.int32, device=dev), scratch, B, T2, F2, C)
    got = xd.cpu()
    assert same(got[2], x[2])
    end = np.array([r[0] + 3, r[1] + 3, T2 + 1])
    real = ConformerTransducer._real_blocks(end, B, T2, F2)
    slack, total = F2 + 2, B * (T2 + 1) * (F2 + 1)
    reach = np.zeros(total, bool)
    for k in np.flatnonzero(real):
        reach[max(0, k * 256 - slack):min(total, (k + 1) * 256 + slack)] = True
    reach = torch.from_numpy(reach).view(B, T2 + 1, F2 + 1)
    for b in (0, 1):
        rb = r[b]
        assert same(got[b, :rb], x[b, :rb])
        terms = x[b, rb:].double()
        S, A, n = terms.sum(0), terms.abs().sum(0), terms.shape[0]
        hl = got[b, rb:rb + 3].double().sum(0)
        err = (hl - S).abs()
        print("utterance", b, "rows", n, "max |hi + mid + lo - S|", float(err.max()), "max |S|", float(S.abs().max()))
        assert bool((err <= 2.0 ** -16 * S.abs() + n * 2.0 ** -24 * A).all())
        assert bool((err <= 2.0 ** -24 * S.abs() + n * 2.0 ** -24 * A).all())  # the third term: what is left is the f32 summation
        assert float((got[b, rb].double() - S).abs().max()) > 2.0 ** -12 * float(S.abs().max())  # one row alone would not do
        need = reach[b, rb + 3:]
        assert int(need.sum()) > 0 and bool((got[b, rb + 3:][need] == 0).all())
        assert bool((got[b, :, 0] == 0).all()) and bool((got[b, 0] == 0).all())
    with pytest.raises(_lib.TfasrUnsupported):
        K.s2d_tail_fold(xd.float(), torch.tensor(r, dtype=torch.int32, device=dev), scratch, B, T2, F2, C)


def test_fold_kernel_leaves_unreachable_rows_and_sums_many_chunks(dev):
    """a tail of several chunks of time rows; rows no computed block reaches may keep stale values, the reachable ones are zero"""
    B, T2, F2, C = 2, 150, 3, 8
    r = [5, 140]
    g = torch.Generator().manual_seed(12)
    x = torch.randn(B, T2 + 1, F2 + 1, C, generator=g).to(BF16)
    x[:, 0] = 0
    x[:, :, 0] = 0
    xd = x.to(dev)
    K.s2d_tail_fold(xd, torch.tensor(r, dtype=torch.int32, device=dev), torch.zeros(B, F2 + 1, C, device=dev), B, T2, F2, C)
    got = xd.cpu()
    real = ConformerTransducer._real_blocks(np.array(r) + 3, B, T2, F2)
    slack, total = F2 + 2, B * (T2 + 1) * (F2 + 1)
    reach = np.zeros(total, bool)
    for k in np.flatnonzero(real):
        reach[max(0, k * 256 - slack):min(total, (k + 1) * 256 + slack)] = True
    reach = torch.from_numpy(reach).view(B, T2 + 1, F2 + 1)
    for b in range(B):
        rb = r[b]
        terms = x[b, rb:].double()
        S, A, n = terms.sum(0), terms.abs().sum(0), terms.shape[0]
        err = (got[b, rb:rb + 3].double().sum(0) - S).abs()
        assert bool((err <= 2.0 ** -16 * S.abs() + n * 2.0 ** -24 * A).all())
        assert same(got[b, :rb], x[b, :rb])
        assert bool((got[b, rb + 3:][reach[b, rb + 3:]] == 0).all())


# ------------------------------------------------------------------------------------------------------------- the K-block table
def ktab_case(M, N, Kd, seed):
    g = torch.Generator().manual_seed(seed)
    nblk = -(-Kd // 256)
    tiles = sorted({0, nblk - 1} | set(range(2, nblk, 3)))
    X = torch.randn(Kd, M, generator=g).to(BF16)
    Y = (torch.randn(Kd, N, generator=g) + 0.2).to(BF16)
    listed = torch.isin(torch.arange(Kd) // 256, torch.tensor(tiles))
    ref = X[listed].double().T @ Y[listed].double()
    refb = Y[listed].double().sum(0)
    Xn, Yn = X.clone(), Y.clone()
    Xn[~listed] = NAN
    Yn[~listed] = NAN
    assert int((~listed).sum()) > 0
    return Xn, Yn, tiles, ref, refb


def ktab_hold(out, gb, ref, refb, alpha, Kd):
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gb).all())
    # the bounds of test_gemm_gpu.py::test_weight_gradient_with_fused_bias_gradient (bf16)
    np.testing.assert_allclose(out.cpu().numpy(), (alpha * ref).numpy(), rtol=2e-2, atol=2e-2 * 70)
    np.testing.assert_allclose(gb.cpu().numpy(), (alpha * refb).numpy(), rtol=1e-3, atol=2e-2 * 70)


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("Kd", [800, 1024, 256 * 37 - 100])
@pytest.mark.parametrize("M,N", [(192, 192), (64, 256)])
def test_k_block_table_single_launch(dev, M, N, Kd, split):
    X, Y, tiles, ref, refb = ktab_case(M, N, Kd, M + Kd)
    out, gb = torch.zeros(M, N, device=dev), torch.zeros(N, device=dev)
    K.gemm(X.to(dev), Y.to(dev), out, M, N, Kd, M, N, N, trans_a=True, accumulate=True, split_k=split, alpha=0.5, colsum=gb,
           k_tiles=torch.tensor(tiles, dtype=torch.int32, device=dev))
    ktab_hold(out, gb, ref, refb, 0.5, Kd)


@pytest.mark.parametrize("Kd", [800, 1024, 256 * 37 - 100])
@pytest.mark.parametrize("M,N", [(192, 192), (64, 256)])
def test_k_block_table_grouped(dev, M, N, Kd):
    calls, want = [], []
    for i in range(3):
        X, Y, tiles, ref, refb = ktab_case(M, N, Kd, 100 * i + Kd)
        out, gb = torch.zeros(M, N, device=dev), torch.zeros(N, device=dev)
        calls.append(dict(A=X.to(dev), B=Y.to(dev), out=out, M=M, N=N, K=Kd, lda=M, ldb=N, ldd=N, trans_a=True, accumulate=True,
                          colsum=gb if i != 1 else None, k_tiles=torch.tensor(tiles, dtype=torch.int32, device=dev)))
        want.append((out, gb, ref, refb))
    before = _lib.load().tfasr_launch_count()
    K.gemm_group(calls)
    assert _lib.load().tfasr_launch_count() - before == 1  # one launch for the three
    for i, (out, gb, ref, refb) in enumerate(want):
        ktab_hold(out, gb, ref, refb if i != 1 else torch.zeros_like(refb), 1.0, Kd)


def test_k_block_table_is_validated(dev):
    M, N, Kd = 192, 192, 1024
    X = torch.zeros(Kd, M, dtype=BF16, device=dev)
    Y = torch.zeros(Kd, N, dtype=BF16, device=dev)
    five = torch.zeros(5, dtype=torch.int32, device=dev)
    out = torch.full((M, N), -7.0, device=dev)
    with pytest.raises(_lib.TfasrError):  # more entries than blocks
        K.gemm(X, Y, out, M, N, Kd, M, N, N, trans_a=True, accumulate=True, k_tiles=five)
    # the product that is not a transposed-A weight gradient: unsupported, nothing launched
    a = K._gemm_args(X.view(M, Kd), Y, out, M, N, Kd, Kd, N, N, accumulate=True)
    a.k_tiles, a.n_k_tiles = five.data_ptr(), 2
    assert _lib.load().tfasr_gemm(ctypes.byref(a), None) == _lib.STATUS_UNSUPPORTED
    with pytest.raises(_lib.TfasrUnsupported):  # ... and with the K-segments of the convolutions
        K.gemm(X, Y, out, M, N, Kd, M, N, N, trans_a=True, accumulate=True, k_tiles=five[:2],
               seg=(torch.zeros(Kd // 64, dtype=torch.int64, device=dev), None, 64))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ------------------------------------------------------------------------------------------------- the row list of the one-pass backward
def test_row_list_of_the_one_pass_backward(dev):
    i = so.bn0_inputs("c64_even", BF16, "random")  # B, T0, F0, C = 3, 37, 80, 64: T1 = 19, F1 = 40
    B, T0, F0 = i["x"].shape
    C = i["w"].shape[-1]
    T1, F1, T2, F2 = so.dims(T0, F0)
    rows = sorted(set(range(0, 7)) | {T1 - 1, T1, T1 + 5, 2 * T1 + 3, 3 * T1 - 1})
    keep = torch.zeros(B * T1, dtype=torch.bool)
    keep[rows] = True
    keep = keep.view(B, T1, 1, 1)
    dy0 = torch.where(keep, i["dy"], torch.zeros((), dtype=BF16))
    dyn = torch.where(keep, i["dy"], torch.full((), NAN, dtype=BF16))
    ref = so.bn0_backward(i["x"], i["w"], i["b"], i["fin"], dy0, i["count"])
    bound = so.bn0_backward_bounds(ref)
    want = torch.cat([ref["P"].reshape(-1), ref["bstats"][:C]])
    x, w, b, fin = (i[k].to(dev) for k in ("x", "w", "b", "fin"))
    res = {}
    for name, dy, rl in (("listed", dyn, torch.tensor(rows, dtype=torch.int32, device=dev)), ("full", dy0, None)):
        dyS = so.to_s2d(dy, fill=NAN).reshape(-1, 4 * C).to(dev)
        bst, pbuf = torch.zeros(2 * C, device=dev), torch.zeros(10 * C, device=dev)
        K.conv1_bn_bwd_onepass_s2d(x, w, b, fin, dyS, bst, pbuf, row_list=rl)
        eb, ep = (bst.cpu().double() - ref["bstats"]).abs(), (pbuf.cpu().double() - want).abs()
        print(name, "bstats error / bound", float((eb / bound["bstats"]).max()), "pbuf error / bound", float((ep / bound["pbuf"]).max()))
        assert bool((eb <= bound["bstats"]).all()) and bool((ep <= bound["pbuf"]).all()), name
        res[name] = (bst, pbuf)
    assert bool(torch.isfinite(res["listed"][1]).all())


# ------------------------------------------------------------------------------------------------------------------------ the model
def batch(dev):
    g = np.random.default_rng(7)
    sig = np.zeros((5, T0 * STEP), np.float32)
    for b, n in enumerate(NSAMP):
        sig[b, :n] = np.clip(g.standard_normal(n) * 0.1, -1, 1)
    fm = np.zeros((5, 1, 2), np.int32)
    fm[2, 0], fm[3, 0] = (10, 7), (60, 20)
    tm = np.zeros((5, 1, 2), np.int32)
    tm[1, 0] = (140, 10)  # ends on utterance 1's last real frame (149)
    tm[0, 0] = (200, 15)
    return torch.from_numpy(sig).to(dev), (torch.from_numpy(fm), torch.from_numpy(tm))


GRADS = ("enc/sub/conv1/w", "enc/sub/conv1/b", "enc/sub/conv0/w", "enc/sub/conv0/b", "enc/sub/bn0/g", "enc/sub/bn0/b")
EARLY = ("enc/sub/bn1/g", "enc/sub/bn1/b")


def run(dev, monkeypatch, switches=(False, True), dtype=BF16, gram=True, foreign=False, **over):
    """one forward of the subsampling, then one backward per switch value from the same saved state and the same gradient; per switch:
    (gradients, what the backward saw)"""
    cfg = configs.conformer_tiny(filters=64, num_blocks=1, **over)
    model = ConformerTransducer(cfg, dev, dtype=dtype, seed=0)
    model._conv1_gram = gram
    sig, masks = batch(dev)
    feats, flen = model.frontend(sig, NSAMP, True, masks)
    if foreign:
        feats = feats.clone()
    ctx = {}
    x0, T2, elen = model._subsampling_fwd(feats, flen, True, ctx)
    g = torch.Generator().manual_seed(5)
    dx0 = (torch.randn(x0.shape, generator=g) * 0.1 + 0.02).to(dtype).to(dev)
    fold, group, gemm = K.s2d_tail_fold, K.gemm_group, K.gemm
    out = {}
    for on in switches:
        model._sub_tail_bwd = on
        for n in GRADS + EARLY:
            model.ps.g(n).zero_()
        seen = {}

        def spy_fold(x, *a, **k):
            seen["do_before"] = x.clone()
            return fold(x, *a, **k)

        def spy_group(calls):
            seen["do"] = calls[0]["B"].clone()
            seen["k_tiles"] = calls[0].get("k_tiles")
            return group(calls)

        def spy_gemm(A, Bm, o, *a, **k):
            r = gemm(A, Bm, o, *a, **k)
            if k.get("bns") is not None:  # the linear layer's data gradient = da2 from its second slot on (the ff = 0 slots are cleared later)
                seen["da2"] = torch.cat([torch.zeros_like(o[:64]), o]).view(5, 101, 21, 64)[:, :, 1:].clone()
            return r

        monkeypatch.setattr(K, "s2d_tail_fold", spy_fold)
        monkeypatch.setattr(K, "gemm_group", spy_group)
        monkeypatch.setattr(K, "gemm", spy_gemm)
        model._subsampling_bwd(dx0, ctx)
        torch.cuda.synchronize()
        monkeypatch.undo()
        out[on] = ({n: model.ps.g(n).clone() for n in GRADS + EARLY}, seen)
    return out, ctx["sub"], model


def float64_reference(s, model, do):
    """the gradients behind `do` (the unfolded gradient w.r.t. conv2's output, S rows) from the tensors the forward saved"""
    B, T0_, F0, T1, F1, T2, F2 = s["dims"]
    C = model.ps.filt_phys
    a1 = so.from_s2d(s["a1"].cpu().double().view(B, T2 + 1, F2 + 1, 2, 2, C), T1, F1)
    dod = do.cpu().double().view(B, T2 + 1, F2 + 1, C)[:, 1:, 1:]
    W = model.ps.w2d("enc/sub/conv1/w").cpu()
    g2 = so.conv2(a1, W, torch.zeros(C), dod)
    w0, b0 = model.ps.p("enc/sub/conv0/w").cpu(), model.ps.p("enc/sub/conv0/b").cpu()
    fin0, count0, _ = s["bn0"]
    g1 = so.bn0_backward(s["feats"].cpu(), w0, b0, fin0.cpu(), g2["dx"], count0)
    return {"enc/sub/conv1/w": g2["dW"].reshape(-1), "enc/sub/conv1/b": g2["db"], "enc/sub/conv0/w": g1["dw_onepass"].reshape(-1),
            "enc/sub/conv0/b": g1["db_onepass"], "enc/sub/bn0/g": g1["bstats"][C:], "enc/sub/bn0/b": g1["bstats"][:C]}


def test_model_switch_on_against_off(dev, monkeypatch):
    out, sub, model = run(dev, monkeypatch)
    (goff, soff), (gon, son) = out[False], out[True]
    assert "do_before" in son and "do_before" not in soff and son["k_tiles"] is not None and soff["k_tiles"] is None
    assert sub["tail_bwd"] is not None and len(sub["tail_bwd"]) == 3
    T2, F2, C = 100, 20, 64
    r = ConformerTransducer._tail_rows(np.array(TF), T0)["o"]
    # in front of the fold.  The linear layer's data gradient has no unordered sum in it: bitwise.
    assert same(son["da2"], soff["da2"])
    # BatchNorm1's backward sums are f32 atomics of up to 1024 partial sums in arrival order (two runs of ONE route differ): dbeta, dgamma
    # and what they feed are held to that reordering, 1024 x 2^-24 of their sums of |terms| (|swish'| <= 1.1), and `do` to one bf16 step more
    fin1, count1 = sub["bn1"]
    da2, o = soff["da2"].float().reshape(-1, C), sub["o"].view(5, T2 + 1, F2 + 1, C)[:, :, 1:].float().reshape(-1, C)
    xh = ((o - fin1[:C]) * fin1[C:2 * C]).abs()
    Ab, Ag = (da2.abs() * 1.1).sum(0), (da2.abs() * 1.1 * xh).sum(0)
    for n, A in (("enc/sub/bn1/b", Ab), ("enc/sub/bn1/g", Ag)):
        d = (gon[n] - goff[n]).abs()
        print(n, "max |on - off|", float(d.max()), "bound", float((2.0 ** -14 * A).min()))
        assert bool((d <= 2.0 ** -14 * A).all()), n
    dob, doff = son["do_before"].float().view(-1, C), soff["do"].float().view(-1, C)
    xh = ((sub["o"].float().view(-1, C) - fin1[:C]) * fin1[C:2 * C]).abs()
    tol = 2.0 ** -7 * doff.abs() + fin1[2 * C:3 * C].abs() / count1 * 2.0 ** -14 * (Ab + xh * Ag)
    print("do before the fold: max |on - off|", float((dob - doff).abs().max()), "elements that differ", int((dob != doff).sum()))
    assert bool(((dob - doff).abs() <= tol).all())
    # the fold itself, inside the switch-on run: rows in front of r and the utterances that are not folded keep their bits
    don, dpre = son["do"].view(5, T2 + 1, F2 + 1, C), son["do_before"].view(5, T2 + 1, F2 + 1, C)
    folded = 0
    for b in range(5):
        if r[b] + 3 <= T2:
            assert same(don[b, :r[b]], dpre[b, :r[b]]) and not same(don[b, r[b]:], dpre[b, r[b]:]), b
            assert bool((don[b, r[b] + 3:r[b] + 5] == 0).all())
            folded += 1
        else:
            assert same(don[b], dpre[b]), b
    assert folded == 3
    # behind it: no further from float64 than twice the full route (two runs of one route differ through unordered f32 atomics)
    # (each run against the float64 gradients of ITS OWN `do`: the two differ by a bf16 step in a few elements, see above)
    ref, ref_on = float64_reference(sub, model, soff["do"]), float64_reference(sub, model, son["do_before"])
    for n in GRADS:
        eon = float((gon[n].cpu().double().reshape(-1) - ref_on[n]).abs().max())
        eoff = float((goff[n].cpu().double().reshape(-1) - ref[n]).abs().max())
        print("PARITY", n, "max|on - f64|", eon, "max|off - f64|", eoff, "max|f64|", float(ref[n].abs().max()))
        assert bool(torch.isfinite(gon[n]).all()), n
        assert eon <= 2 * eoff, n


@pytest.mark.parametrize("case", ["f32", "layer_norm", "two_pass", "foreign_features"])
def test_fallbacks_take_the_full_route(dev, monkeypatch, case):
    kw = dict(f32=dict(dtype=torch.float32), layer_norm=dict(sub_norm="layer"), two_pass=dict(gram=False), foreign_features=dict(foreign=True))[case]
    out, sub, _ = run(dev, monkeypatch, **kw)
    (goff, soff), (gon, son) = out[False], out[True]
    assert "do_before" not in son and son.get("k_tiles") is None and sub.get("tail_bwd") is None
    # one route run twice: unordered f32 atomics in the BatchNorm sums may move a bf16 intermediate by one step (2^-8) - of the largest
    # element, or, for conv2's bias gradient (the column sums of `do`, which BatchNorm1's backward makes cancel), of its sum of |terms|
    for n in GRADS:
        a, b = gon[n].double(), goff[n].double()
        scale = float(b.abs().max())
        if n == "enc/sub/conv1/b" and "do" in soff:
            scale = float(soff["do"].double().abs().view(-1, b.numel()).sum(0).max())
        if n == "enc/sub/conv0/b" and sub.get("s2d"):  # scale x (sum dz - its mean x N - ...): BatchNorm0 makes the terms cancel
            C = b.numel()
            scale = float((sub["bn0"][0][2 * C:3 * C].double().abs() * goff["enc/sub/bn0/b"].double().abs()).max())
        assert bool(torch.isfinite(a).all()), n
        assert float((a - b).abs().max()) <= 2.0 ** -8 * scale + 1e-30, n
