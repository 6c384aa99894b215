"""GPU parity of the RNN-T loss on the kernel branches the Conformer configurations never reach (csrc/rnnt_loss.hip, rnnt_impl):

  A. the lattice dispatch edges: rnnt_lattice_wave_kernel<1|2|4> with lane 63 occupied (U1 = 64, 128, 256), one column past each edge
     (65, 129, 257) and the workgroup kernel rnnt_lattice_kernel (257 <= U1 <= 1024, up to 1024 threads);
  B. the packed lattice (row stride Ul+1, not the U1 that picks the kernel) on the E = 2 / E = 4 wave kernels and the workgroup kernel;
  C. the vocabulary paths: second 512-column register chunk, V = 1024 (upper edge of the register path and of the streamed gradient),
     V > 1024 (online (max, sum) loop + cross-lane merge, vector branch of rnnt_grad_kernel), scalar paths, bf16 on every one of them;
  D. the kernels' own input clamps (lengths, label ids, empty utterance) and the U1 > 1024 refusal.

Reference: oracle/rnnt_ref.rnnt_loss_and_grad in float64.  Tolerances are the project's existing pairs (tests/test_rnnt_gpu.py):
costs rtol=1e-5, atol=1e-4; f32 gradients rtol=5e-4, atol=2e-5 (test_vs_oracle_ragged) up to U1 = 256 and rtol=1e-2, atol=1e-4
(test_reference_smoke_shape's long f32 lattice) above: on these inputs the float32 NumPy oracle itself sits at 0.75x of the tight pair
at U1 = 513 and 1.02x at U1 = 1024 (no room left for the kernel's own error), at most 0.07x of the loose pair, and at most 0.21x of
the tight pair up to U1 = 256; bf16: cost rtol=1e-3, gradients rtol=2e-2, atol=4e-3 (test_bf16_within_north_star_tolerance).
Measured margins of the kernels and of the float32 oracle, case by case: profiles/rnnt_loss_paths_parity.json.

Sensitivity (checked once with two value-only mutations of a scratch build): an alpha pass of rnnt_lattice_kernel that gives column
512 no left neighbour fails exactly the U1 = 513 and 1024 cases of group A; a vector branch of rnnt_grad_kernel without the blank
column's patch fails exactly V = 1032 and 2048 of group C.  (With a draw that sends 1e-7 of the mass through the last column the
U1 = 513 case did NOT notice the first one: hence the last-column condition in test_lattice_dispatch_edges and the fixed seeds.)
"""
import functools

import numpy as np
import pytest
import torch

from oracle import rnnt_ref
from tensorflowasr_amd import _lib, kernels

pytestmark = pytest.mark.gpu

COST_TOL = dict(rtol=1e-5, atol=1e-4)
GRAD_TOL_F32 = dict(rtol=5e-4, atol=2e-5)        # test_vs_oracle_ragged
GRAD_TOL_F32_LONG = dict(rtol=1e-2, atol=1e-4)   # test_reference_smoke_shape (U1 > 256)
COST_TOL_BF16 = dict(rtol=1e-3, atol=0.0)        # test_bf16_within_north_star_tolerance
GRAD_TOL_BF16 = dict(rtol=2e-2, atol=4e-3)


def _run(dev, logits, labels, ul, tl, dtype=torch.float32, grad_scale=None, inplace=False):
    d = lambda a, t: torch.from_numpy(np.array(a, t)).to(dev)  # (a copy: the shared case arrays are read-only)
    lg = d(logits, np.float32).to(dtype).contiguous()
    gs = None if grad_scale is None else d(grad_scale, np.float32)
    costs, grads = kernels.rnnt_loss_fwd_bwd(lg, d(labels, np.int32), d(ul, np.int32), d(tl, np.int32), grad_scale=gs,
                                             grads=lg if inplace else None)
    torch.cuda.synchronize()
    return costs.cpu().numpy(), grads.float().cpu().numpy()


def ratio(got, want, rtol, atol):
    """worst |got - want| / (atol + rtol |want|): what np.testing.assert_allclose compares with 1"""
    want = np.asarray(want, np.float64)
    return float((np.abs(np.asarray(got, np.float64) - want) / (atol + rtol * np.abs(want))).max())


def _check(tag, loss, grads, ref_loss, ref_g, cost_tol, grad_tol):
    print(f"\n[rnnt paths] {tag} cost_ratio={ratio(loss, ref_loss, **cost_tol):.4f} grad_ratio={ratio(grads, ref_g, **grad_tol):.4f}")
    np.testing.assert_allclose(loss, ref_loss, **cost_tol)
    np.testing.assert_allclose(grads, ref_g, **grad_tol)


# ------------------------------------------------------------------------------------------------------------- A
LATTICE_CASES = [  # (B, T, U1, V), seed
    ((3, 9, 64, 24), 22262),                                                            # wave E=1, lane 63 live
    ((3, 9, 65, 8), 30265), ((3, 9, 128, 8), 12808),                                    # wave E=2: first column past E=1, lane 63 live
    ((3, 9, 129, 8), 12908), ((3, 9, 256, 8), 41446),                                   # wave E=4
    ((3, 6, 257, 8), 33627), ((3, 5, 513, 8), 90903), ((3, 7, 1024, 8), 102408), ((2, 40, 300, 16), 30016),  # workgroup kernel
]


@functools.lru_cache(maxsize=None)
def lattice_case(shape, seed):
    """Inputs + float64 reference of one group-A case (computed once, shared, read-only).
    Utterance 0 is full (Tl = T, Ul = U1-1: the last column of the last lane / thread is live), utterance 1 has Ul = 0, utterance 2 is
    ragged with Ul % 4 != 0 (the lattice ends inside a lane's E columns); at U1 = 64 and 300 one more utterance is appended with
    Tl = 1, Ul = U1-1 (a single time row: ndiag = U1)."""
    B, T, U1, V = shape
    U = U1 - 1
    ul2 = 2 * U // 3
    while ul2 % 4 == 0:
        ul2 -= 1
    tl = [T, T - 1, T - 2][:B]
    ul = [U, 0, ul2][:B]
    if U1 in (64, 300):
        tl.append(1)
        ul.append(U)
    tl, ul = np.array(tl, np.int32), np.array(ul, np.int32)
    B = len(tl)
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, T, U1, V)) * 1.5).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    logits[np.arange(B)[:, None, None], np.arange(T)[None, :, None], np.arange(U)[None, None, :], labels[:, None, :]] += 3.0
    scale = rng.uniform(0.5, 2.0, B)
    ref_loss, ref_g = rnnt_ref.rnnt_loss_and_grad(logits, labels, ul, tl)
    for a in (logits, labels, tl, ul, scale, ref_loss, ref_g):
        a.setflags(write=False)
    return logits, labels, ul, tl, scale, ref_loss, ref_g


def live_fraction(ref_g, ul, tl):
    """share of the valid lattice nodes whose reference gradient row has an entry above 1e-3"""
    B, T, U1, _ = ref_g.shape
    valid = (np.arange(T)[None, :, None] < tl[:, None, None]) & (np.arange(U1)[None, None, :] <= ul[:, None, None])
    live = (np.abs(ref_g) > 1e-3).any(-1)
    assert not (live & ~valid).any()
    return (live & valid).sum() / valid.sum()


@pytest.mark.parametrize("shape,seed", LATTICE_CASES, ids=["B%d-T%d-U1_%d-V%d" % s for s, _ in LATTICE_CASES])
def test_lattice_dispatch_edges(dev, shape, seed):
    logits, labels, ul, tl, scale, ref_loss, ref_g = lattice_case(shape, seed)
    U1 = shape[2]
    assert ul[0] == U1 - 1 and tl[0] == shape[1] and ul[1] == 0 and (len(ul) < 3 or ul[2] % 4)
    # non-vacuity, on the reference alone: the lattice carries gradient mass, not a handful of nodes
    frac = live_fraction(ref_g, ul, tl)
    print(f"\n[rnnt paths] A/U1_{U1} live_fraction={frac:.3f}")
    assert frac >= 0.10
    # ... and the LAST column's alpha is observable: its terminal node has g_blank = -1 whatever alpha is, so a node above it must carry
    # gradient far over the tolerance (100 x the loose atol).  Seeds that send ~1e-7 of the mass there leave the last thread unchecked.
    want = ref_g * scale[:, None, None, None]
    last = np.abs(want[0, :shape[1] - 1, U1 - 1]).max()
    print(f"[rnnt paths] A/U1_{U1} last_column_mass={last:.3e}")
    assert last >= 1e-2
    loss, grads = _run(dev, logits, labels, ul, tl, grad_scale=scale)
    _check(f"A/B{shape[0]}-T{shape[1]}-U1_{U1}-V{shape[3]}", loss, grads, ref_loss, want, COST_TOL,
           GRAD_TOL_F32 if U1 <= 256 else GRAD_TOL_F32_LONG)
    loss2, g2 = _run(dev, logits, labels, ul, tl, grad_scale=scale, inplace=True)
    np.testing.assert_array_equal(loss2, loss)
    np.testing.assert_array_equal(g2, grads)


# ------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("U1m", [130, 300])
def test_packed_lattice_long_rows(dev, U1m, dtype):
    """tfasr_rnnt_loss_packed == the dense entry where U1 selects the E = 4 wave kernel (130) and the workgroup kernel (300), with
    packed row strides Ul+1 = U1m, 1, 65 (the E = 2 range) and 4."""
    B, T, U, V = 4, 7, U1m - 1, 8
    rng = np.random.default_rng(U1m)
    logits = (rng.standard_normal((B, T, U + 1, V)) * 1.5).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    ul = np.array([U, 0, 64, 3], np.int32)
    tl = np.array([7, 1, 5, 7], np.int32)
    scale = rng.uniform(0.5, 2, B).astype(np.float32)
    d = lambda a: torch.from_numpy(a).to(dev)
    dense = d(logits).to(dtype)
    costs_d, g_d = kernels.rnnt_loss_fwd_bwd(dense, d(labels), d(ul), d(tl), grad_scale=d(scale))
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum(tl.astype(np.int64) * (ul + 1))
    packed = torch.cat([dense[b, :tl[b], :ul[b] + 1].reshape(-1, V) for b in range(B)]).contiguous()
    costs_p, g_p = kernels.rnnt_loss_packed(packed, d(labels), d(ul), d(tl), d(off), int(off[-1]), T, grad_scale=d(scale))
    torch.cuda.synchronize()
    np.testing.assert_allclose(costs_p.cpu().numpy(), costs_d.cpu().numpy(), rtol=1e-6)
    want = torch.cat([g_d[b, :tl[b], :ul[b] + 1].reshape(-1, V) for b in range(B)])
    np.testing.assert_array_equal(g_p.float().cpu().numpy(), want.float().cpu().numpy())
    ref_loss, _ = rnnt_ref.rnnt_loss_and_grad(dense.float().cpu().numpy(), labels, ul, tl)
    np.testing.assert_allclose(costs_p.cpu().numpy(), ref_loss, rtol=1e-3 if dtype == torch.bfloat16 else 1e-5)


# ------------------------------------------------------------------------------------------------------------- C
VOCAB_CASES = [(V, dt) for V in (520, 1024, 1032, 2048, 1027) for dt in ("f32", "bf16")] + [(7, "bf16"), (129, "bf16")]
VOCAB_EDGE_LABELS = (0, 7, 8, 511, 512, 1023, 1024)  # chunk and 8-group boundaries of the pick / patch code; 0 = the blank's own column


def vocab_labels(V):
    """[2, 6] labels fixed by hand: every edge id below V and V-1 sits on a LIVE node (utterance 0: six labels, utterance 1: two)."""
    req = [v for v in VOCAB_EDGE_LABELS if v < V]
    if V - 1 not in req:
        req.append(V - 1)
    fill = [(3 + 5 * i) % V for i in range(12)]
    live = (req + fill)[:8]
    labels = np.array([live[:6], live[6:8] + fill[8:12]], np.int32)
    assert set(req) <= set(labels[0]) | set(labels[1, :2])
    return labels


@functools.lru_cache(maxsize=None)
def vocab_case(V, dt):
    B, T, U1 = 2, 6, 7
    rng = np.random.default_rng(V)
    logits = (rng.standard_normal((B, T, U1, V)) * 1.5).astype(np.float32)
    if dt == "bf16":
        logits = torch.from_numpy(logits).to(torch.bfloat16).float().numpy()  # the oracle sees the same rounded inputs
    labels = vocab_labels(V)
    tl, ul = np.array([6, 4], np.int32), np.array([6, 2], np.int32)
    scale = rng.uniform(0.5, 2.0, B)
    ref_loss, ref_g = rnnt_ref.rnnt_loss_and_grad(logits, labels, ul, tl)
    for a in (logits, labels, tl, ul, scale, ref_loss, ref_g):
        a.setflags(write=False)
    return logits, labels, ul, tl, scale, ref_loss, ref_g


@pytest.mark.parametrize("V,dt", VOCAB_CASES, ids=lambda p: str(p))
def test_vocabulary_paths(dev, V, dt):
    logits, labels, ul, tl, scale, ref_loss, ref_g = vocab_case(V, dt)
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    loss, grads = _run(dev, logits, labels, ul, tl, dtype=dtype, grad_scale=scale)
    _check(f"C/V{V}/{dt}", loss, grads, ref_loss, ref_g * scale[:, None, None, None], COST_TOL_BF16 if dt == "bf16" else COST_TOL,
           GRAD_TOL_BF16 if dt == "bf16" else GRAD_TOL_F32)
    loss2, g2 = _run(dev, logits, labels, ul, tl, dtype=dtype, grad_scale=scale, inplace=True)
    np.testing.assert_array_equal(loss2, loss)
    np.testing.assert_array_equal(g2, grads)


# ------------------------------------------------------------------------------------------------------------- D
def _clamp_inputs(U1):
    B, T, V = 3, 6, 8
    rng = np.random.default_rng(U1)
    logits = (rng.standard_normal((B, T, U1, V)) * 1.5).astype(np.float32)
    labels = rng.integers(1, V, (B, U1 - 1)).astype(np.int32)
    scale = rng.uniform(0.5, 2.0, B)
    return B, T, V, logits, labels, scale


@pytest.mark.parametrize("U1", [10, 300])
def test_overlong_lengths_are_clamped(dev, U1):
    """logit_len > T and label_len > U1-1 mean T and U1-1: min(logit_len, T), min(label_len, U1-1) in every kernel."""
    B, T, V, logits, labels, scale = _clamp_inputs(U1)
    want = _run(dev, logits, labels, [U1 - 1, U1 // 2, U1 - 1], [T, T - 2, T], grad_scale=scale)
    got = _run(dev, logits, labels, [U1 + 3, U1 // 2, U1 + 3], [T + 5, T - 2, T + 5], grad_scale=scale)
    assert np.isfinite(want[0]).all() and (want[0] > 0).all()
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("U1", [10, 300])
def test_out_of_range_labels_are_clamped(dev, U1):
    """label ids below 0 mean 0 (the blank's column: both patches land on x[0]), ids above V-1 mean V-1."""
    B, T, V, logits, labels, scale = _clamp_inputs(U1)
    ul, tl = [U1 - 1, U1 // 2, U1 - 1], [T, T - 2, T]
    bad, good = labels.copy(), labels.copy()
    lo, hi = [0, 2, U1 // 2 - 1, U1 - 2], [1, 3, U1 // 2 - 2, U1 - 3]  # first / last live columns of all three utterances
    bad[:, lo], good[:, lo] = -3, 0
    bad[:, hi], good[:, hi] = V + 9, V - 1
    want = _run(dev, logits, good, ul, tl, grad_scale=scale)
    got = _run(dev, logits, bad, ul, tl, grad_scale=scale)
    ref_loss, ref_g = rnnt_ref.rnnt_loss_and_grad(logits, good, np.array(ul), np.array(tl))
    np.testing.assert_allclose(want[0], ref_loss, **COST_TOL)  # label id 0 itself against the oracle
    np.testing.assert_allclose(want[1], ref_g * scale[:, None, None, None], **(GRAD_TOL_F32 if U1 <= 256 else GRAD_TOL_F32_LONG))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


@pytest.mark.parametrize("U1", [10, 300])
def test_empty_utterance_between_two_normal_ones(dev, U1):
    """logit_len = 0: cost exactly 0, gradient all zero, and the neighbours are what they are without it."""
    B, T, V, logits, labels, scale = _clamp_inputs(U1)
    loss, grads = _run(dev, logits, labels, [U1 - 1, 0, U1 // 2], [T, 0, T - 1], grad_scale=scale)
    assert loss[1] == 0.0 and not np.signbit(loss[1])
    assert not grads[1].any()
    keep = [0, 2]
    loss2, grads2 = _run(dev, logits[keep], labels[keep], [U1 - 1, U1 // 2], [T, T - 1], grad_scale=scale[keep])
    assert np.isfinite(loss2).all() and (loss2 > 0).all() and np.abs(grads2).max() > 0.1
    np.testing.assert_array_equal(loss[keep], loss2)
    np.testing.assert_array_equal(grads[keep], grads2)


def test_u1_above_1024_is_rejected(dev):
    """U1 = 1025 has no lattice kernel: TFASR_STATUS_INVALID_VALUE, check() raises, nothing is launched, costs / grads stay untouched."""
    B, T, U1, V = 1, 1, 1025, 8
    logits = torch.zeros(B, T, U1, V, device=dev)
    labels = torch.ones(B, U1 - 1, dtype=torch.int32, device=dev)
    ul = torch.tensor([U1 - 1], dtype=torch.int32, device=dev)
    tl = torch.tensor([T], dtype=torch.int32, device=dev)
    grads = torch.full_like(logits, 7.25)
    n0 = kernels.launch_count()
    with pytest.raises(_lib.TfasrError, match=r"rnnt_loss: .*\(status 1\)"):
        kernels.rnnt_loss_fwd_bwd(logits, labels, ul, tl, grads=grads)
    costs = torch.full((B,), 7.25, device=dev)
    ws = kernels.workspace(kernels.rnnt_loss_workspace_size(B, T, U1, V), dev, "rnnt")
    p = kernels._p
    st = _lib.load().tfasr_rnnt_loss(p(logits), p(grads), p(labels), p(ul), p(tl), None, B, T, U1, V, 0, _lib.TFASR_F32, p(costs), p(ws),
                                     ws.numel(), kernels._stream())
    torch.cuda.synchronize()
    assert st == 1  # TFASR_STATUS_INVALID_VALUE
    assert kernels.launch_count() == n0
    assert (costs == 7.25).all() and (grads == 7.25).all()
    # the largest U1 the entry accepts, for contrast
    c, _ = kernels.rnnt_loss_fwd_bwd(logits[:, :, :1024].contiguous(), labels[:, :1023].contiguous(), ul - 1, tl)
    assert torch.isfinite(c).all() and kernels.launch_count() > n0
