"""tests/dwconv_oracle.py (the float64 reference of tests/test_dwconv_gpu.py) against torch autograd on the expressions of
oracle/conformer_ref.py, in float64; and the GPU suite's own cases, checks and bounds run on a plain-torch EMULATION of the kernels'
arithmetic (float32 accumulation, bf16 storage at the rounding points dwconv_oracle.py lists) instead of the GPU:
    the emulation stays inside every bound on every random case, and equals the reference bit for bit on every exact case (whose values
    are asserted to be representable in their storage type): the reference and the bounds are sound on their own;
    each of eight index faults seeded into the emulation breaks an exact case and exceeds a bound on a random case: the suite would notice.
Runs without a GPU."""
import numpy as np
import pytest
import torch

import dwconv_oracle as DO
import test_dwconv_gpu as G
from oracle import conformer_ref as R

BF, F32 = torch.bfloat16, torch.float32


def close(a, b):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-11, atol=1e-12)


# ----------------------------------------------------------------------------------------------------- the oracle against autograd
@pytest.mark.parametrize("B,T,C,Kk", [(2, 7, 3, 5), (3, 4, 2, 1), (2, 3, 4, 6), (1, 1, 2, 4), (2, 37, 3, 32), (3, 30, 2, 32), (2, 33, 5, 31)])
@pytest.mark.parametrize("bias", [False, True])
def test_depthwise_conv_against_autograd(B, T, C, Kk, bias):
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + Kk)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x, w, b, dy = r(B, T, C).requires_grad_(True), r(Kk, C).requires_grad_(True), r(C).requires_grad_(True) if bias else None, r(B, T, C)
    y = R.depthwise_conv1d_causal(x, w, b)
    y.backward(dy)
    f, bd, bw = DO.dwconv_fwd(x, w, b), DO.dwconv_bwd_data(dy, w), DO.dwconv_bwd_weight(x, dy, Kk)
    close(f["y"], y)
    close(bd["dx"], x.grad)
    close(bw["dw"], w.grad)
    close(bw["dbias"], b.grad if bias else dy.sum((0, 1)))
    for res, names in ((f, ["y"]), (bd, ["dx"]), (bw, ["dw", "dbias"])):
        for n in names:
            assert (res["M_" + n] >= res[n].abs() - 1e-12).all()


def test_glu_against_autograd():
    g = torch.Generator().manual_seed(5)
    x, dg = torch.randn(3, 5, 16, generator=g, dtype=torch.float64).requires_grad_(True), torch.randn(3, 5, 8, generator=g, dtype=torch.float64)
    y = x[..., :8] * torch.sigmoid(x[..., 8:])
    y.backward(dg)
    close(DO.glu_fwd(x)["g"], y)
    b = DO.glu_bwd(x, dg)
    close(b["d"], x.grad)
    assert (b["M_d"] >= b["d"].abs() - 1e-12).all()
    assert torch.equal(DO.glu_bwd(x, dg, 2 * dg.abs())["M_d"], 2 * b["M_d"])


def test_statistics_and_their_copies():
    g = torch.Generator().manual_seed(6)
    y = torch.randn(3, 70, 4, generator=g, dtype=torch.float64)
    t = DO.bn_stats_of(y)
    close(t["stats"], torch.cat([y.sum((0, 1)), (y * y).sum((0, 1))]))
    for ncopy in (1, 3, 8):
        c = DO.bn_stats_copies(y, ncopy)
        close(c["stats"].sum(0), t["stats"])
        close(c["M_stats"].sum(0), t["M_stats"])
    one = torch.zeros(3, 70, 4, dtype=torch.float64)
    one[2, 64, 1] = 3.0  # utterance 2, time tile 2 of 32 steps -> copy (2 + 2) % 3 = 1
    c = DO.bn_stats_copies(one, 3)["stats"]
    assert float(c[1, 1]) == 3.0 and float(c[1, 5]) == 9.0 and float(c.abs().sum()) == 12.0
    assert DO.stats_copy_of(3, 70, 3).tolist() == [[0, 1, 2], [1, 2, 0], [2, 0, 1]]


def test_batchnorm_prologue_adds_the_copies_up():
    inp = G.make_bnin((2, 9, 8, 5, 4, True))
    p = DO.bn_bwd_prologue(inp["bn_x"], inp["dsw"], inp["fin"], inp["bstats"], inp["count"])
    q = G.NO.bn_bwd_apply(inp["bn_x"], inp["dsw"], inp["fin"], inp["bstats"].double().sum(0), inp["count"], act_swish=True)
    close(p["dcv"], q["dx"])


# ------------------------------------------------------------------------------------------------------------------ the emulation
def _gather(x, idx, valid):
    """x [B, T, C] float32, idx / valid [B, T] (rows of the flattened [B * T, C]) -> [B, T, C], zero where not valid"""
    B, T, C = x.shape
    return x.reshape(B * T, C)[idx.clamp(0, B * T - 1)] * valid[..., None].float()


def emu_fwd(x, w, bias, fault=None, rounded=True):
    B, T, C = x.shape
    Kk = w.shape[0]
    xf, t = x.float(), torch.arange(T)
    acc = torch.zeros(B, T, C) + (0.0 if bias is None else bias)
    for k in range(Kk):
        ti = t - (Kk - 1) + k
        if fault == "halo off by one row":  # the rows in front of the 32-step tile come from one row too early
            ti = torch.where(ti < t // (2 * G.TGD) * (2 * G.TGD), ti - 1, ti)
        gi = ti[None, :] + T * torch.arange(B)[:, None]
        ok = ((ti < T)[None, :] & (gi >= 0)) if fault == "window across the utterance boundary" else ((ti >= 0) & (ti < T))[None, :].expand(B, T)
        if fault == "last row of a 16-step group dropped" and k == Kk - 1:  # the newest input row of the group never reaches its output
            ok = ok & (t % G.TGD != G.TGD - 1)[None, :]
        acc = acc + w[k] * _gather(xf, gi, ok)
    return acc.to(x.dtype) if rounded else acc


def emu_bwd_data(dy, w, fault=None, rounded=True):
    B, T, C = dy.shape
    Kk = w.shape[0]
    df, t = dy.float(), torch.arange(T)
    acc = torch.zeros(B, T, C)
    for k in range(Kk):
        ti = t + (Kk - 1) - k
        gi = ti[None, :] + T * torch.arange(B)[:, None]
        acc = acc + w[Kk - 1 - k if fault == "taps not reversed" else k] * _gather(df, gi, (ti < T)[None, :].expand(B, T))
    return acc.to(dy.dtype) if rounded else acc


def emu_bwd_weight(x, dy, dw0, db0, fault=None):
    """per 64-step workgroup tile a float32 partial sum, the partial sums added up in float32, added to dw0 / db0"""
    B, T, C = x.shape
    Kk = dw0.shape[0]
    xf, df, t = x.float(), dy.float(), torch.arange(T)
    dw, db = torch.zeros(Kk, C), torch.zeros(C)
    for t0 in range(0, T, 2 * G.TG):
        sl = slice(t0, min(t0 + 2 * G.TG, T))
        d = df[:, sl].clone()
        if fault == "one 32-step tile counted twice":
            d[0, :G.TG] *= 2 if t0 == 0 else 1
        for k in range(Kk):
            ti = t[sl] - (Kk - 1) + k
            gi = ti[None, :] + T * torch.arange(B)[:, None]
            xs = _gather(xf, gi, (ti >= 0)[None, :].expand(B, ti.numel()))
            dw[k] += (d * xs).sum((0, 1))
        db += ((xf[:, sl] if fault == "dbias taken from x" else d)).sum((0, 1))
    return dw0 + dw, None if db0 is None else db0 + db


def emu_stats(y, st0, fault=None):
    ncopy = st0.shape[0]
    B, T, C = y.shape
    cp, yf, st = DO.stats_copy_of(B, T, ncopy), y.float(), st0.clone()
    for b in range(B):
        for j in range(cp.shape[1]):
            if fault == "one statistics copy dropped" and cp[b, j] == ncopy - 1:
                continue
            rows = yf[b, j * 2 * G.TGD:(j + 1) * 2 * G.TGD]
            st[cp[b, j]] += torch.cat([rows.sum(0), (rows * rows).sum(0)])
    return st


def _halves(x, fault):
    C = x.shape[-1] // 2
    a, b = x[..., :C].float(), x[..., C:].float()
    return (b, a) if fault == "GLU halves swapped" else (a, b)


def emu_glu_fwd(x, fault=None):
    a, b = _halves(x, fault)
    return (a * torch.sigmoid(b)).to(x.dtype)


def emu_glu_bwd(x, dg, fault=None):
    """dg float32 (the unrounded data gradient of the fused kernels) or the storage type"""
    a, b = _halves(x, fault)
    s, d = torch.sigmoid(b), dg.float()
    return torch.cat([d * s, d * a * s * (1.0 - s)], -1).to(x.dtype)


def emu_conv(case, inp, fault=None):
    return dict(y=emu_fwd(inp["x"], inp["w"], inp["bias"], fault), dx=emu_bwd_data(inp["dy"], inp["w"], fault))


def emu_wgrad(case, inp, fault=None):
    dw, db = emu_bwd_weight(inp["x"], inp["dy"], inp["dw0"], inp["db0"], fault)
    return dict(dw=dw, dbias=db)


def emu_many(case, inps, fault=None):
    r = [emu_wgrad(None, i, fault) for i in inps]
    return dict(dw=[o["dw"] for o in r], dbias=[o["dbias"] for o in r])


def emu_fwd_stats(case, inp, fault=None):
    y = emu_fwd(inp["x"], inp["w"], inp["bias"], fault)
    return dict(y=y, stats=emu_stats(y, inp["st0"], fault))


def emu_gin(case, inp, fault=None):
    gt = emu_glu_fwd(inp["glu_x"], fault)
    y = emu_fwd(gt, inp["w"], inp["bias"], fault)
    return dict(g=gt, y=y, stats=emu_stats(y, inp["st0"], fault))


def emu_bwd_glu(case, inp, fault=None):
    return dict(dglu=emu_glu_bwd(inp["glu_x"], emu_bwd_data(inp["dy"], inp["w"], fault, rounded=False), fault))


def emu_bnin(case, inp, fault=None):
    C = case[2]
    mean, rstd, sc, sh = inp["fin"].reshape(4, C)
    s = inp["bstats"].sum(0)
    inv = torch.tensor(1.0 / inp["count"], dtype=F32)
    qq = sc * rstd * s[C:] * inv
    cb, cd = -qq, qq * mean - sc * s[:C] * inv
    x, d = inp["bn_x"].float(), inp["dsw"].float()
    z = x * sc + sh
    sg = torch.sigmoid(z)
    dcv = (sc * (d * (sg * (1.0 + z * (1.0 - sg)))) + cb * x + cd).to(BF)
    dglu = emu_glu_bwd(inp["glu_x"], emu_bwd_data(dcv, inp["w"], fault, rounded=False), fault)
    grads = inp["dg0"] is not None
    return dict(dcv=dcv, dglu=dglu, dgamma=inp["dg0"] + inp["gscale"] * s[C:] if grads else None, dbeta=inp["db0"] + inp["gscale"] * s[:C] if grads else None)


def emu_glu(case, inp, fault=None):
    return dict(g=emu_glu_fwd(inp["x"], fault), d=emu_glu_bwd(inp["x"], inp["dg"], fault))


KINDS = ("exact", "random")
# family -> (cases, kinds, make(case, kind), emulate(case, inp, fault), check(case, kind, inp, out))
FAMILIES = {
    "conv": (G.CONV_SIZES + G.CONV_SEAMS + G.CONV_SLABS + G.CONV_SCALAR, KINDS, G.make_conv, emu_conv, G.check_conv),
    "wgrad": (G.WGRAD_TILE + G.WGRAD_FALLBACK, KINDS, G.make_wgrad, emu_wgrad, G.check_wgrad),
    "many": (G.MANY_CASES + G.MANY_FALLBACK, KINDS, G.make_many, emu_many, G.check_many),
    "fwd_stats": (G.FWD_STATS_CASES, KINDS, G.make_fwd_stats, emu_fwd_stats, G.check_fwd_stats),
    "gin": (G.GIN_CASES, KINDS, G.make_gin, emu_gin, G.check_gin),
    "bwd_glu": (G.BWD_GLU_CASES, KINDS, G.make_bwd_glu, emu_bwd_glu, G.check_bwd_glu),
    "bnin": (G.BNIN_CASES, ("random",), lambda case, kind: G.make_bnin(case), emu_bnin, lambda case, kind, inp, out: G.check_bnin(case, inp, out)),
    "glu": (G.GLU_SMALL, KINDS, G.make_glu, emu_glu, G.check_glu),
    "glu past one trip": (G.GLU_BIG, ("random",), G.make_glu, emu_glu, G.check_glu),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_emulation_stays_inside_every_bound_and_equals_every_exact_case(family):
    """the GPU suite's cases and checks on the emulation: random cases inside the bounds (worst ratio per bound printed), exact cases bit
    for bit, their reference values representable in the storage type (asserted by the checks themselves)"""
    cases, kinds, make, emulate, check = FAMILIES[family]
    del G.RATIOS[:]
    for case in cases:
        for kind in kinds:
            inp = make(case, kind)
            check(case, kind, inp, emulate(case, inp))
    worst = {}
    for what, r in G.RATIOS:
        worst[what] = max(worst.get(what, 0.0), r)
    assert worst, "no bound was exercised"
    for what, r in sorted(worst.items()):
        print(f"emulation, {family}: worst max |emulation - ref| / bound of {what} = {r:.3g}")
        assert r < 1


FAULTS = {  # fault seeded into the emulation -> the families whose checks must catch it
    "halo off by one row": ("conv",),
    "window across the utterance boundary": ("conv", "fwd_stats"),
    "last row of a 16-step group dropped": ("conv", "gin"),
    "one 32-step tile counted twice": ("wgrad", "many"),
    "taps not reversed": ("conv", "bwd_glu"),
    "one statistics copy dropped": ("fwd_stats", "gin"),
    "GLU halves swapped": ("glu", "gin", "bwd_glu"),
    "dbias taken from x": ("wgrad",),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_seeded_index_fault_breaks_an_exact_case_and_exceeds_a_bound(fault):
    for family in FAULTS[fault]:
        cases, kinds, make, emulate, check = FAMILIES[family]
        caught = {}
        for kind in kinds:
            for case in cases:
                inp = make(case, kind)
                try:
                    check(case, kind, inp, emulate(case, inp, fault))
                except AssertionError:
                    caught[kind] = case
                    break
        print(f"{fault}: {family}: exact case {caught.get('exact')}, random case {caught.get('random')}")
        assert set(caught) == set(kinds), f"{fault} passed every {set(kinds) - set(caught)} case of {family}"
