"""GPU: the fused attention backward as ONE launch of both sides (tfasr_relattn_bwd_prep + tfasr_relattn_fused_bwd_qk) against the two
launches it replaces (tfasr_relattn_fused_bwd_q3, then tfasr_relattn_fused_bwd_k) on the same inputs.

Everything a workgroup OWNS is bitwise the same: q + u, q + v and both planes of dvec (the preparation kernel runs the query-side kernel's
prologue arithmetic), dq, dk, dv and the stored unskewed dS; the key side's sample order (longest first) is checked to be the permutation
the header promises.  The u / v bias gradients and the bias row of the table gradient are f32 atomics of per-workgroup sums - their order
differs between two runs of either route - and are held to the bound tests/test_ops_gpu.py::test_relattn_fused_backward_v2_no_skewed_gradient
gives the same quantities (3e-2 relative, 3e-2 of the largest element absolute)."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer

pytestmark = pytest.mark.gpu

ATOMIC_TOL = 3e-2  # test_ops_gpu.py `close`: the bound of du / dv / dpext there


def _inputs(dev, B, H, T, dh_logical, seed):
    g = torch.Generator().manual_seed(seed)
    HD = H * 64
    keep = (torch.arange(64) < dh_logical).repeat(H)  # a head of `dh_logical` dims stored zero-padded to 64
    qkv = (torch.randn(B * T, 3 * HD, generator=g) * 0.7 * keep.repeat(3)).to(torch.bfloat16)
    u, v = torch.randn(HD, generator=g) * 0.3 * keep, torch.randn(HD, generator=g) * 0.3 * keep
    pext = (torch.randn(2 * T, HD, generator=g) * 0.7 * keep).to(torch.bfloat16)
    dout = (torch.randn(B * T, HD, generator=g) * keep).to(torch.bfloat16)
    return qkv.to(dev), u.to(dev), v.to(dev), pext.to(dev), dout.to(dev)


CASES = [
    # B, T, lengths, logical head size, chunk, history
    pytest.param(3, 150, (150, 70, 1), 64, None, None, id="BH12-partial-block-one-sample-padding"),
    pytest.param(2, 65, (65, 64), 64, None, None, id="block-boundary-two-blocks"),
    pytest.param(9, 130, (130,) * 9, 64, None, None, id="B9-all-equal"),
    pytest.param(9, 130, (90, 130, 64, 130, 17, 64, 129, 1, 100), 64, None, None, id="B9-two-ties"),
    pytest.param(4, 150, (3, 66, 128, 150), 64, None, None, id="ascending-order-reverses"),
    pytest.param(3, 150, (150, 70, 1), 36, None, None, id="heads-36-as-64"),
    pytest.param(3, 150, (150, 70, 1), 64, 16, 64, id="streaming-16-64"),
]


@pytest.mark.parametrize("B,T,lens,dhl,chunk,hist", CASES)
def test_merged_launch_equals_the_two_launches(dev, B, T, lens, dhl, chunk, hist):
    H, dh = 4, 64
    HD = H * dh
    scale = 1.0 / float(np.sqrt(dhl))
    win = dict(chunk_size=chunk, history_size=hist)
    qkv, u, v, pext, dout = _inputs(dev, B, H, T, dhl, seed=T * 31 + B)
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    o, lse = K.relattn_fused_fwd(qkv, u, v, pext, ln, B, H, T, dh, scale, use_mask=True, **win)
    lds = -(-T // 8) * 8

    def fresh():
        return dict(dqkv=torch.zeros(B * T, 3 * HD, dtype=torch.bfloat16, device=dev), du=torch.zeros(HD, device=dev), dv=torch.zeros(HD, device=dev),
                    dpext=torch.zeros(2 * T, HD, device=dev), ds=torch.zeros(B, H, T, lds, dtype=torch.bfloat16, device=dev))

    a = fresh()  # the two launches
    _, dvec_a, qu_a, qv_a = K.relattn_fused_bwd_q3(qkv, u, v, pext, ln, o, dout, lse, a["dqkv"], a["du"], a["dv"], a["dpext"], B, H, T, dh, scale,
                                                   use_mask=True, ds=a["ds"], **win)
    K.relattn_fused_bwd_k(qkv, qu_a, qv_a, pext, ln, dout, lse, dvec_a, a["dqkv"], B, H, T, dh, scale, use_mask=True, **win)
    b = fresh()  # preparation + the merged launch
    qu_b, qv_b, dvec_b, order = K.relattn_bwd_prep(qkv, u, v, pext, ln, o, dout, B, H, T, dh, use_mask=True)
    K.relattn_fused_bwd_qk(qkv, u, v, pext, ln, dout, lse, qu_b, qv_b, dvec_b, order, b["dqkv"], b["du"], b["dv"], b["dpext"], B, H, T, dh, scale,
                           use_mask=True, ds=b["ds"], **win)
    torch.cuda.synchronize()

    # the key side's order: by length descending, ties by sample index
    want = sorted(range(B), key=lambda s: (-min(lens[s], T), s))
    assert order.cpu().tolist() == want and sorted(want) == list(range(B))
    # rows of a wholly padded 64-query block are written by neither route (and read by nobody)
    live = torch.zeros(B, T, dtype=torch.bool)
    for s, n in enumerate(lens):
        live[s, :min(-(-n // 64) * 64, T)] = True
    rows = live.view(B * T).to(dev)
    assert torch.equal(qu_b[rows], qu_a[rows]) and torch.equal(qv_b[rows], qv_a[rows])
    lv = live[:, None, :].expand(B, H, T).to(dev)
    for plane in range(2):
        assert torch.equal(dvec_b[plane][lv].view(torch.int32), dvec_a[plane][lv].view(torch.int32)), f"dvec plane {plane}"
    assert torch.isfinite(a["dqkv"].float()).all()
    assert torch.equal(b["dqkv"][:, :HD], a["dqkv"][:, :HD]), "dq"
    assert torch.equal(b["dqkv"][:, HD:2 * HD], a["dqkv"][:, HD:2 * HD]), "dk"
    assert torch.equal(b["dqkv"][:, 2 * HD:], a["dqkv"][:, 2 * HD:]), "dv"
    assert float(a["dqkv"][:, HD:].float().abs().max()) > 0 and float(a["dqkv"][:, :HD].float().abs().max()) > 0
    assert torch.equal(b["ds"].view(torch.int16), a["ds"].view(torch.int16)), "dS"
    for name in ("du", "dv", "dpext"):
        x, y = b[name].cpu().numpy(), a[name].cpu().numpy()
        np.testing.assert_allclose(x, y, rtol=ATOMIC_TOL, atol=ATOMIC_TOL * float(np.abs(y).max()), err_msg=name)


def test_block_backward_same_with_the_merged_launch_on_and_off(dev, monkeypatch):
    """One Conformer block (S dims, heads 36 stored as 64) through the native block executor, backward at B = 2, T' = 150 with
    TFASR_ATTN_BWD_QK = 0 / 1.  What the attention backward owns (dq, dk, dv, dS) is bitwise the same on the same inputs - the cases above -
    but a block's input gradient is not a bitwise quantity even between two runs of ONE route: the ConvModule's BatchNorm sums above the
    attention are f32 atomics, and a sum that rounds the other way flips bf16 elements of the input gradient by a whole ulp (2^-7 of the
    element; measured: 22 of 43 200 elements between two runs of the two-launch route, and two equal runs followed by a third that
    differed).  So the input gradient is held to the bound tests/test_parity_baseline_gpu.py puts on a block's input gradient through
    two routes (relative L2 5e-3) and the f32 parameter gradients to the bound tests/test_block_hoist_gpu.py allows two orders of the same
    f32 sums (2e-3 of the largest gradient); the two-launch route is run twice so that its own spread is printed beside the difference."""
    B, T, d = 2, 150, 144
    lens = [150, 70]
    cfg = configs.conformer_s(dropout=0.0, num_blocks=1)
    model = ConformerTransducer(cfg, dev, dtype=torch.bfloat16, seed=1)
    assert model.ps.head_phys == 64 and model._fused_attention() and model.native_blocks
    g = torch.Generator().manual_seed(0)
    xd = torch.randn(B * T, d, generator=g).to(dev).to(torch.bfloat16)
    dyd = (torch.randn(B * T, d, generator=g) * 0.1).to(dev).to(torch.bfloat16)
    elen_dev = torch.tensor(lens, dtype=torch.int32, device=dev)
    outs = []
    for switch in ("0", "0", "1"):
        monkeypatch.setenv("TFASR_ATTN_BWD_QK", switch)
        model.zero_grad()
        cx = {}
        model._block_fwd_native(xd, 0, B, T, elen_dev, True, cx)
        dx = model._block_bwd_native(dyd, 0, cx)
        torch.cuda.synchronize()
        outs.append((dx.clone(), model.ps.grad.clone()))
    (dx0, g0), (dx0b, _), (dx1, g1) = outs
    assert torch.isfinite(dx1.float()).all() and float(dx1.float().abs().max()) > 0
    rel = float((dx1.double() - dx0.double()).norm() / dx0.double().norm())
    own = float((dx0b.double() - dx0.double()).norm() / dx0.double().norm())
    print(f"\n[attn bwd qk] block input gradient, relative L2: merged vs two launches {rel:.3e}, two launches vs themselves {own:.3e}")
    assert rel < 5e-3, rel
    np.testing.assert_allclose(g1.cpu().numpy(), g0.cpu().numpy(), rtol=0, atol=2e-3 * float(g0.abs().max()))
