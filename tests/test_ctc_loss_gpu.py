"""CTC loss, gradient and greedy decoding (csrc/ctc.hip) at real lattice sizes and at the edges, against oracle/ctc_ref.py in float64.

Every case runs in f32 and bf16; the oracle sees the logits already rounded to the storage type, so the comparison measures the
kernels' arithmetic and not the rounding of their input.

Bars.  Cost: the project's bars (tests/test_ctc.py), rtol 2e-5 in f32 and 1e-3 in bf16.  Gradient: the error of a float32 log-space
lattice is the cancellation in alpha + beta - lp - logP with |alpha| in the thousands, it grows with T and no fixed atol fits both a
20-frame and a 1000-frame case.  The yardstick is therefore the oracle's own float32 run of the same case (as in
tests/test_attn_plain_gpu.py): err32 = max |oracle f32 - oracle f64|, at least 2e-5 (the atol tests/test_ctc.py asks), and
    f32:   max |got - want| <= 4 err32                     (4: the project's allowance for another summation order)
    bf16:  |got - want| <= 4 err32 + 2^-8 |want|  elementwise  (the stored result is rounded to nearest, 2^-9 relative, times 2)
with both sides multiplied by the row's grad_scale.  (bf16 keeps 8 significant bits, so just above a power of two rounding alone
comes close to 2^-8 |want|: a bf16 ratio of 0.9 at a short case is the store, not the lattice; the f32 run of the case shows that.)  Every measured error and its bar is printed before it is asserted and goes to
profiles/ctc_loss_parity.json.

Rows without frames (cost 0 without labels, +inf with, gradient zero) and rows whose labels do not fit their frames (cost +inf,
gradient exactly zero; the oracle's gradient is NaN there) are stated by definition, like the reference golden.  Every other row's
float64 cost is asserted finite before the kernel is looked at: a case whose reference is infeasible has the wrong seed, not a
lenient bar.  Lengths beyond the padding, a negative label length (an empty one, as in csrc/align.hip) and labels outside [0, V)
are compared with the oracle on the clamped values."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

from oracle import ctc_ref
from tensorflowasr_amd import kernels as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
COST_RTOL = {"f32": 2e-5, "bf16": 1e-3}  # north_star: CTC loss within 1e-3 relative
ERR32_FLOOR = 2e-5
I32 = torch.int32


def _wave(T, U, V):
    return dict(shape=(3, T, U, V), ul=[U, U // 2 + 1, 1], tl=[T, T - 1, max(3, T // 3)])


def _edit_beyond(labels):
    labels[1, 1] = 9  # >= V: class V-1
    labels[3, 0] = -3  # < 0: class 0
    labels[0, 2] = 6  # == V


def _edit_degenerate(labels):
    labels[4, 1] = labels[4, 0]  # two equal labels in two frames: no room for the blank between them


# name: shape (B, T, U, V), logit scale (2), blank (0), ul / tl (None: ragged, feasible by construction), edit(labels), rows that are
# infeasible by construction
LOSS_CASES = {
    # the state scan around its wave boundaries: S = 2U+1 = 63 | 65, 127 | 129, 255 | 257, 1023 (the widest workgroup)
    "wave_1_U31": _wave(70, 31, 8),
    "wave_2_U32": _wave(70, 32, 8),
    "wave_2_U63": _wave(140, 63, 8),
    "wave_3_U64": _wave(140, 64, 8),
    "wave_4_U127": _wave(300, 127, 12),
    "wave_5_U128": _wave(300, 128, 12),
    "wave_16_U511": _wave(1023, 511, 16),
    # production sizes; scale 4 is the sharp posterior of a trained model
    "bench": dict(shape=(8, 250, 64, 1000)),
    "long_sharp": dict(shape=(4, 900, 300, 1000), scale=4.0),
    # 36000 rows: the per-frame pass strides its grid above 32768
    "grid_stride": dict(shape=(40, 900, 20, 29)),
    # the wave reduction over V; at V = 2 every adjacent pair of labels is a repeat
    "V2": dict(shape=(2, 12, 4, 2), ul=[4, 4], tl=[12, 8]),
    "V5": dict(shape=(2, 12, 4, 5), ul=[4, 4], tl=[12, 8]),
    "V63": dict(shape=(2, 12, 4, 63), ul=[4, 4], tl=[12, 8]),
    "V64": dict(shape=(2, 12, 4, 64), ul=[4, 4], tl=[12, 8]),
    "V65": dict(shape=(2, 12, 4, 65), ul=[4, 4], tl=[12, 8]),
    "V16384": dict(shape=(1, 8, 3, 16384), ul=[3], tl=[8]),  # the limit kernels.ctc_loss_fwd_bwd states
    "blank0": dict(shape=(3, 70, 33, 17), ul=[33, 17, 1], tl=[70, 69, 23]),
    "blank8": dict(shape=(3, 70, 33, 17), ul=[33, 17, 1], tl=[70, 69, 23], blank=8),
    "blank16": dict(shape=(3, 70, 33, 17), ul=[33, 17, 1], tl=[70, 69, 23], blank=16),
    "degenerate": dict(shape=(5, 12, 4, 7), ul=[4, 0, 0, 3, 2], tl=[12, 5, 0, 0, 2], edit=_edit_degenerate, infeasible=(4,)),
    "beyond_padding": dict(shape=(5, 10, 4, 6), ul=[7, 4, -1, 2, 3], tl=[14, 10, 10, 9, 11], blank=2, edit=_edit_beyond),
}
VARIANT_CASE = "blank0"
_REF = {}  # (case, dtype) -> the inputs and the oracle's answer, computed once and shared
_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def parity_profile():
    yield
    if {f"{c}/{d}" for c in LOSS_CASES for d in DTYPES} <= set(_PARITY):  # (a partial run leaves the file alone)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "ctc_loss_parity.json"), "w") as f:
            json.dump({"what": "tfasr_ctc_loss against oracle/ctc_ref.py in float64 on the rounded logits (tests/test_ctc_loss_gpu.py): "
                               "cost_err = max relative error of the finite costs; grad_err = max |got - want|; err32 = the same for the "
                               "oracle in float32 (at least 2e-5); grad_bar = 4 err32 (bf16: + 2^-8 |want| elementwise); grad_ratio = "
                               "worst error / bar over the elements",
                       "cases": {k: _PARITY[k] for k in sorted(_PARITY)}}, f, indent=1)
            f.write("\n")


def _reference(case, dname):
    """the case's inputs and the float64 answer: dict(x, labels, ul, tl, scale, blank, cost, grad (unscaled), err32)"""
    if (case, dname) in _REF:
        return _REF[case, dname]
    c = LOSS_CASES[case]
    B, T, U, V = c["shape"]
    blank = c.get("blank", 0)
    rng = np.random.default_rng([zlib.crc32(case.encode()), B, T, U, V])
    x = torch.from_numpy((rng.standard_normal((B, T, V)) * c.get("scale", 2.0)).astype(np.float32)).to(DTYPES[dname])
    labels = rng.integers(0, V - 1, (B, U)).astype(np.int32)
    labels += labels >= blank  # uniform in the non-blank classes
    if c.get("edit"):
        c["edit"](labels)
    lab_c = np.clip(labels, 0, V - 1)
    if c.get("ul") is None:
        ul = rng.integers(1, U + 1, B).astype(np.int32)
        ul[0] = U
        need = [int(ul[b] + (lab_c[b, 1:ul[b]] == lab_c[b, :ul[b] - 1]).sum()) for b in range(B)]
        tl = np.array([rng.integers(n, T + 1) for n in need], np.int32)
        tl[0] = T
    else:
        ul, tl = np.array(c["ul"], np.int32), np.array(c["tl"], np.int32)
    ul_c, tl_c = np.clip(ul, 0, U), np.clip(tl, 0, T)
    cost, grad = np.zeros(B), np.zeros((B, T, V))
    rows = [b for b in range(B) if tl_c[b] > 0 and b not in c.get("infeasible", ())]
    for b in range(B):
        if b not in rows:
            cost[b] = 0.0 if (tl_c[b] == 0 and ul_c[b] == 0) else np.inf
    xr = x.float().numpy()[rows]
    cost[rows], grad[rows] = ctc_ref.ctc_loss_and_grad(xr, lab_c[rows], ul_c[rows], tl_c[rows], blank)
    assert np.isfinite(cost[rows]).all(), (case, cost)  # the reference of every such row is feasible
    _, g32 = ctc_ref.ctc_loss_and_grad(xr, lab_c[rows], ul_c[rows], tl_c[rows], blank, dtype=torch.float32)
    err32 = max(float(np.abs(g32.astype(np.float64) - grad[rows]).max()), ERR32_FLOOR)
    for b in range(B):
        grad[b, tl_c[b]:] = 0.0
    assert np.isfinite(grad).all()
    scale = rng.uniform(0.5, 2, B).astype(np.float32)
    _REF[case, dname] = dict(x=x, labels=labels, ul=ul, tl=tl, ul_c=ul_c, tl_c=tl_c, scale=scale, blank=blank, cost=cost, grad=grad,
                             err32=err32, rows=rows)
    return _REF[case, dname]


def _run(dev, r, **kw):
    out = K.ctc_loss_fwd_bwd(r["x"].to(dev), torch.from_numpy(r["labels"]).to(dev), torch.from_numpy(r["ul"]).to(dev),
                             torch.from_numpy(r["tl"]).to(dev), blank=r["blank"], **kw)
    torch.cuda.synchronize()
    return out


def _grad_check(got, want, err32, scale, dname):
    """-> (max abs error, worst error / bar); want is unscaled"""
    sc = scale.astype(np.float64)[:, None, None]
    want = want * sc
    bar = 4 * err32 * sc + (2.0 ** -8 * np.abs(want) if dname == "bf16" else 0.0)
    err = np.abs(got.double().cpu().numpy() - want)
    return float(err.max()), float((err / bar).max())


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", list(LOSS_CASES))
def test_ctc_loss_and_gradient_against_float64_oracle(dev, case, dname):
    r = _reference(case, dname)
    if case == "degenerate":  # without labels only the all-blank path is left
        lp = torch.log_softmax(r["x"][1, :5].double(), -1)[:, r["blank"]]
        assert abs(r["cost"][1] + float(lp.sum())) < 1e-9
        assert r["cost"].tolist()[2:] == [0.0, np.inf, np.inf]
    costs, grads = _run(dev, r, grad_scale=torch.from_numpy(r["scale"]).to(dev))
    assert grads.dtype == DTYPES[dname] and grads.shape == r["x"].shape
    costs, fin = costs.double().cpu().numpy(), np.isfinite(r["cost"])
    cost_err = float((np.abs(costs[fin] - r["cost"][fin]) / np.maximum(np.abs(r["cost"][fin]), 1e-30)).max()) if fin.any() else 0.0
    gerr, ratio = _grad_check(grads, r["grad"], r["err32"], r["scale"], dname)
    print(f"{case}/{dname}: cost error {cost_err:.3e} (bar {COST_RTOL[dname]:.0e}), gradient error {gerr:.3e} (f32 oracle {r['err32']:.3e}, "
          f"bar 4x{' + 2^-8 |want|' if dname == 'bf16' else ''}), worst error / bar {ratio:.3f}")
    _PARITY[f"{case}/{dname}"] = dict(cost_err=cost_err, cost_bar=COST_RTOL[dname], grad_err=gerr, err32=r["err32"], grad_bar=4 * r["err32"],
                                      grad_ratio=ratio)
    np.testing.assert_allclose(costs, r["cost"], rtol=COST_RTOL[dname], atol=0)  # (+inf equals +inf, 0 equals 0)
    assert torch.isfinite(grads.float()).all()
    assert ratio <= 1.0
    g = grads.float().cpu().numpy()
    for b in range(len(costs)):
        assert not g[b, r["tl_c"][b]:].any()  # exactly zero past the row's frames
        if not fin[b]:
            assert not g[b].any()  # ... and everywhere in a row that cannot be aligned


@pytest.mark.parametrize("dname", list(DTYPES))
def test_ctc_loss_call_variants(dev, dname):
    """want_grads=False, grad_scale=None, a caller's grads buffer, and a second call.  Costs are bit-equal between calls.  Gradients
    are NOT asserted bit-equal: ctc_grad_kernel sums the occupancies of a repeated label with LDS float atomics, whose order is not
    fixed; two such sums of at most U terms that add up to at most 1 differ by at most U 2^-23 (and by one bf16 step once stored)."""
    r = _reference(VARIANT_CASE, dname)
    B, T, U, V = LOSS_CASES[VARIANT_CASE]["shape"]
    ones = np.ones(B, np.float32)
    costs, grads = _run(dev, r, grad_scale=torch.from_numpy(ones).to(dev))
    costs2, none = _run(dev, r, want_grads=False)
    assert none is None and torch.equal(costs, costs2)
    costs3, grads3 = _run(dev, r)  # grad_scale=None
    assert torch.equal(costs, costs3)
    tol = dict(rtol=2.0 ** -7, atol=U * 2.0 ** -23) if dname == "bf16" else dict(rtol=0, atol=U * 2.0 ** -23)
    np.testing.assert_allclose(grads3.float().cpu().numpy(), grads.float().cpu().numpy(), **tol)
    for g in (grads, grads3):
        gerr, ratio = _grad_check(g, r["grad"], r["err32"], ones, dname)
        print(f"{VARIANT_CASE}/{dname}: gradient error {gerr:.3e}, worst error / bar {ratio:.3f}")
        assert ratio <= 1.0
    buf = torch.full((B, T, V), 777.0, dtype=DTYPES[dname], device=dev)
    costs4, grads4 = _run(dev, r, grads=buf)
    assert grads4.data_ptr() == buf.data_ptr() and torch.equal(costs, costs4)
    assert not (buf == 777.0).any() and torch.isfinite(buf.float()).all()  # every element written, frames past logit_len too
    for b in range(B):
        assert not buf[b, int(r["tl_c"][b]):].any()
    np.testing.assert_allclose(buf.float().cpu().numpy(), grads.float().cpu().numpy(), **tol)


# ------------------------------------------------------------------------------------------------------------------ greedy decoder
def _greedy_check(dev, x, tl, blank):
    """x: torch [B,T,V] in the storage type; tokens and lengths exactly as the oracle on the same values"""
    toks, n = K.ctc_greedy_decode(x.to(dev), torch.as_tensor(np.asarray(tl, np.int32)).to(dev), blank=blank)
    torch.cuda.synchronize()
    rt, rn = ctc_ref.ctc_greedy_decode(x.float().numpy(), np.clip(tl, 0, x.shape[1]), blank)
    np.testing.assert_array_equal(n.cpu().numpy(), rn)
    np.testing.assert_array_equal(toks.cpu().numpy(), rt)  # the padding past the token count is `blank`
    return rt, rn


@pytest.mark.parametrize("dname", list(DTYPES))
def test_ctc_loss_greedy_ties_take_the_lowest_index(dev, dname):
    """Equal maxima in different lanes, in one lane's stride (v and v + 64), and at index 0 and V-1: the lowest index wins, as np.argmax."""
    V, blank = 200, 7
    ties = [(3, 10), (5, 69), (10, 3), (69, 133, 5), (0, V - 1), (63, 64), (V - 1, 0, 64), (130, 131, 194), (1, 65, 129, 193),
            (blank, 20), (2, blank), tuple(range(V))]  # no two neighbours with the same answer: nothing merges
    rng = np.random.default_rng(17)
    x = np.clip(rng.standard_normal((2, len(ties), V)) * 2, -7, 7).astype(np.float32)
    for t, idx in enumerate(ties):
        x[0, t, list(idx)] = 8.0  # exact in bf16
        x[1, t, list(idx)] = -7.0  # ... and a tie below everything else changes nothing
    x[1, :, 150] = 7.5
    xt = torch.from_numpy(x).to(DTYPES[dname])
    am = xt.float().numpy().argmax(-1)
    assert am[0].tolist() == [min(i) for i in ties]
    rt, rn = _greedy_check(dev, xt, [len(ties), len(ties)], blank)
    assert rn.tolist() == [len(ties) - 1, 1] and rt[1, 0] == 150  # (one frame is the blank)


def test_ctc_loss_greedy_ties_from_bf16_rounding(dev):
    rng = np.random.default_rng(23)
    xt = torch.from_numpy((rng.standard_normal((4, 100, 1000)) * 2).astype(np.float32)).to(torch.bfloat16)
    xf = xt.float().numpy()
    assert ((xf == xf.max(-1, keepdims=True)).sum(-1) > 1).sum() >= 10  # rounding ties the maximum in many rows
    _greedy_check(dev, xt, [100, 37, 100, 1], 0)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("last_blank", [False, True])
@pytest.mark.parametrize("V", [2, 29, 63, 64, 65, 1000])
def test_ctc_loss_greedy_shapes_and_lengths(dev, V, last_blank, dname):
    B, T, blank = 4, 20, (V - 1 if last_blank else 0)
    rng = np.random.default_rng([V, blank])
    x = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
    x[3, :, blank] = 30.0  # an all-blank row
    xt = torch.from_numpy(x).to(DTYPES[dname])
    rt, rn = _greedy_check(dev, xt, [T, 0, 7, T], blank)
    assert rn[0] > 0 and rn[1] == 0 and rn[3] == 0 and (rt[1] == blank).all() and (rt[3] == blank).all()
    _greedy_check(dev, xt, [T + 5, -1, 1, T], blank)  # lengths beyond the padding and below zero


@pytest.mark.parametrize("dname", list(DTYPES))
def test_ctc_loss_greedy_grid_stride_rows(dev, dname):
    B, T, V = 40, 900, 29
    rng = np.random.default_rng(36000)
    xt = torch.from_numpy((rng.standard_normal((B, T, V)) * 2).astype(np.float32)).to(DTYPES[dname])
    tl = rng.integers(0, T + 1, B)
    tl[0], tl[B - 1] = T, T
    _greedy_check(dev, xt, tl, 0)


@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("last_blank", [False, True])
def test_ctc_loss_greedy_carry_over_chunks_equals_whole_utterance(dev, last_blank, dname):
    """B = 4 streams of T = 50 cut at random points (empty chunks and a cut between two equal classes among them): the chunks' tokens
    concatenated are the whole-utterance decode, last_class is the class of the stream's last frame so far, and an empty chunk
    leaves it alone."""
    B, T, V, R = 4, 50, 5, 7
    blank = V - 1 if last_blank else 0
    c = 1 if blank != 1 else 2
    rng = np.random.default_rng([5, blank])
    x = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
    x[1, 20:22, c] = 30.0  # two equal non-blank classes, cut between them
    x[2, 30:32, blank] = 30.0  # and two blanks
    xt = torch.from_numpy(x).to(DTYPES[dname])
    am = xt.float().numpy().argmax(-1)
    cuts = np.sort(rng.integers(0, T + 1, (B, R - 1)), axis=1)
    cuts[0, 2] = cuts[0, 1]  # an empty chunk in the middle
    cuts[1] = np.sort(np.r_[21, rng.integers(0, T + 1, R - 2)])
    cuts[2] = np.sort(np.r_[31, 31, rng.integers(0, T + 1, R - 3)])
    cuts[3, 0], cuts[3, -1] = 0, T  # empty first and last chunks
    cuts = np.concatenate([np.zeros((B, 1), int), np.sort(cuts, axis=1), np.full((B, 1), T)], axis=1)
    assert (np.diff(cuts, axis=1) == 0).sum() >= 4 and 21 in cuts[1]
    whole, whole_n = _greedy_check(dev, xt, [T] * B, blank)
    last = torch.full((B,), -1, dtype=I32, device=dev)
    got = [[] for _ in range(B)]
    for k in range(R):
        lens = cuts[:, k + 1] - cuts[:, k]
        Tc = max(int(lens.max()), 1)
        chunk = torch.full((B, Tc, V), 9.0, dtype=DTYPES[dname])  # what lies past a stream's chunk is not looked at
        for b in range(B):
            chunk[b, :lens[b]] = xt[b, cuts[b, k]:cuts[b, k + 1]]
        toks, n = K.ctc_greedy_decode_carry(chunk.to(dev), torch.from_numpy(lens.astype(np.int32)).to(dev), last, blank=blank)
        torch.cuda.synchronize()
        toks, n = toks.cpu().numpy(), n.cpu().numpy()
        for b in range(B):
            got[b] += toks[b, :n[b]].tolist()
            assert (toks[b, n[b]:] == blank).all()
        want_last = [int(am[b, cuts[b, k + 1] - 1]) if cuts[b, k + 1] > 0 else -1 for b in range(B)]
        assert last.cpu().tolist() == want_last, k  # (an empty chunk: the value of the chunk before it)
    for b in range(B):
        assert got[b] == whole[b, :whole_n[b]].tolist(), b
