"""The inference LSTM recurrence (csrc/lstm_infer.hip) over one and two directions against the float64 oracle of tests/ds2_oracle.py:
the persistent launch (bf16), the per-step route (f32, bf16 with the persistent kernels switched off, shapes outside their range).
Bars: bf16 those of tests/test_lstm_persist_gpu.py (rtol 3e-2 / atol 2e-2, the cell state 3e-2 / 3e-2) against the oracle on the
bf16-rounded operands with h carried in bf16; f32 rtol 1e-4 / atol 1e-5."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

import ds2_oracle as DO

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 32), (3, 5, 96), (17, 37, 64), (33, 9, 512), (64, 5, 512)]
BAR = {torch.float32: (dict(rtol=1e-4, atol=1e-5), dict(rtol=1e-4, atol=1e-5)),
       torch.bfloat16: (dict(rtol=3e-2, atol=2e-2), dict(rtol=3e-2, atol=3e-2))}


def _lengths(B, T):
    """always T, then 1 and 0 where B allows, a middle value, the rest spread over 0 .. T"""
    want = [T, 1, 0, (T + 1) // 2]
    lens = [want[b] if b < len(want) else (b * 7) % (T + 1) for b in range(B)]
    return torch.tensor(lens, dtype=torch.int32)


def _case(B, T, P, ndir, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    xg = (torch.randn(B, T, ndir * 4 * P, generator=g) * 0.7).to(dtype)
    rk = (torch.randn(ndir, P, 4 * P, generator=g) * (1.0 / np.sqrt(P))).to(dtype)
    return xg, rk, _lengths(B, T)


def _check(dev, B, T, P, ndir, dtype, persistent):
    xg, rk, lens = _case(B, T, P, ndir, dtype, seed=1000 * B + P + ndir)
    ws = torch.zeros(K.lstm_infer_workspace_size(B, T, P, ndir, K._dt(xg)), dtype=torch.uint8, device=dev)
    y, h, c = K.lstm_infer_fwd(xg.to(dev), rk.to(dev), lens.to(dev), ndir=ndir, want_state=True, ws=ws)
    torch.cuda.synchronize()
    if persistent:
        rec = ws[:ndir * 64].view(torch.int32).cpu().view(ndir, 16)
        assert rec[:, 1].tolist() == [0] * ndir, "a hand-off wait timed out"
        assert rec[:, 0].tolist() == [(P // 16) * (T - 1)] * ndir  # every workgroup arrived after every step but the last: this route ran
    y_ref, h_ref, c_ref = DO.lstm_infer(xg.double(), rk.double(), lens, ndir, hround=DO.bf16_round if dtype == torch.bfloat16 else None)
    ybar, cbar = BAR[dtype]
    np.testing.assert_allclose(y.float().cpu().numpy(), y_ref.numpy(), **ybar)
    np.testing.assert_allclose(h.cpu().numpy(), h_ref.numpy(), **ybar)   # the state at the last valid step
    np.testing.assert_allclose(c.cpu().numpy(), c_ref.numpy(), **cbar)
    yc = y.cpu()
    for b in range(B):
        assert not yc[b, int(lens[b]):].any(), b  # masked outputs are exactly zero
    if int(lens.min()) == 0:
        b = int(lens.argmin())
        assert not yc[b].any() and not h[:, b].any() and not c[:, b].any()  # a row of length 0: zeros throughout, the zero state
    return xg, rk, lens, y


def _reverse_by_length(t, lens):
    out = t.clone()
    for b, n in enumerate(lens.tolist()):
        out[b, :n] = t[b, :n].flip(0)
    return out


@pytest.mark.parametrize("B,T,P", SHAPES)
@pytest.mark.parametrize("ndir", [1, 2])
def test_persistent_launch_bf16(dev, B, T, P, ndir):
    prev = K.lstm_set_persist(1)
    try:
        xg, rk, lens, y = _check(dev, B, T, P, ndir, torch.bfloat16, persistent=True)
        if ndir == 2:
            # direction 1 is bit-equal to a one-direction call on the by-length-reversed projections, reversed back: masked steps leave
            # the state untouched, so the arithmetic is the same
            xr = _reverse_by_length(xg[:, :, 4 * P:].contiguous(), lens)
            y1 = K.lstm_infer_fwd(xr.to(dev), rk[1:2].contiguous().to(dev), lens.to(dev), ndir=1)
            torch.cuda.synchronize()
            assert torch.equal(_reverse_by_length(y1.cpu(), lens), y[:, :, P:].cpu())
            y0 = K.lstm_infer_fwd(xg[:, :, :4 * P].contiguous().to(dev), rk[0:1].contiguous().to(dev), lens.to(dev), ndir=1)
            assert torch.equal(y0.cpu(), y[:, :, :P].cpu())
    finally:
        K.lstm_set_persist(prev)


@pytest.mark.parametrize("B,T,P", SHAPES)
@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_route(dev, B, T, P, ndir, dtype):
    prev = K.lstm_set_persist(0)
    try:
        xg, rk, lens, y = _check(dev, B, T, P, ndir, dtype, persistent=False)
        if ndir == 2:
            xr = _reverse_by_length(xg[:, :, 4 * P:].contiguous(), lens)
            y1 = K.lstm_infer_fwd(xr.to(dev), rk[1:2].contiguous().to(dev), lens.to(dev), ndir=1)
            torch.cuda.synchronize()
            assert torch.equal(_reverse_by_length(y1.cpu(), lens), y[:, :, P:].cpu())
    finally:
        K.lstm_set_persist(prev)


@pytest.mark.parametrize("B,T,P", [(1, 2, 32),      # MT 1: two workgroups, one k-step, a single hand-off
                                   (17, 9, 64),     # MT 2: one row into the second batch tile
                                   (33, 7, 96),     # MT 3: an odd number of k-steps
                                   (64, 5, 128)])   # MT 4: every row of the last tile live
def test_persistent_launch_is_the_training_forward(dev, B, T, P):
    """One direction, zero initial state: the inference kernel is the training forward (csrc/lstm_persist.hip) with the training buffers
    removed - same fragment loads, staging, MFMA order, gate expressions and roundings - so y, the last carried h and the last c agree
    bit for bit, and both launches count (P/16) * (T-1) arrivals on the hand-off of csrc/lstm_handoff.h."""
    xg, rk, lens = (v.to(dev) for v in _case(B, T, P, 1, torch.bfloat16, seed=2000 * B + P))
    bf = torch.bfloat16
    gates = torch.empty(B, T, 4 * P, dtype=bf, device=dev)
    cseq = torch.empty(B, T, P, dtype=torch.float32, device=dev)
    hseq = torch.empty(B, T, P, dtype=bf, device=dev)
    yseq = torch.empty(B, T, P, dtype=bf, device=dev)
    sync = K.lstm_persist_sync(dev)
    ws = torch.zeros(K.lstm_infer_workspace_size(B, T, P, 1, K._dt(xg)), dtype=torch.uint8, device=dev)
    prev = K.lstm_set_persist(1)
    try:
        y, h_last, c_last = K.lstm_infer_fwd(xg, rk, lens, ndir=1, want_state=True, ws=ws)
        K.lstm_persist_fwd(xg, rk[0], None, None, lens, gates, cseq, hseq, yseq, sync)
        torch.cuda.synchronize()
    finally:
        K.lstm_set_persist(prev)
    arrivals = (P // 16) * (T - 1)
    assert ws[:64].view(torch.int32)[:2].tolist() == [arrivals, 0]  # {count, abort}: the persistent route ran, no wait timed out
    assert sync[:2].tolist() == [arrivals, 0]
    assert torch.equal(y, yseq)
    assert torch.equal(h_last[0], hseq[:, -1].float())
    assert torch.equal(c_last[0], cseq[:, -1])


@pytest.mark.parametrize("ndir", [1, 2])
def test_shape_outside_the_persistent_range(dev, ndir):
    """B = 65, P = 48: neither fits the persistent kernels; the entry point takes the per-step kernels by itself"""
    _check(dev, 65, 6, 48, ndir, torch.bfloat16, persistent=False)
