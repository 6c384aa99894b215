"""The inference LSTM recurrence continued from a state (tfasr_lstm_infer_fwd_state, csrc/lstm_infer.hip): the persistent launch (bf16) and
the per-step route (f32, and bf16 with the persistent kernels switched off) against the float64 recurrence with an initial state
(tests/ds2_stream_oracle.py), and the property the DeepSpeech2 session rests on: a sequence walked in several calls gives the bits of one
call over all of it.  Bars: those of tests/test_lstm_infer_gpu.py for the same kernels (bf16 rtol 3e-2 / atol 2e-2, the cell state
3e-2 / 3e-2, against the oracle on the bf16-rounded operands with h carried in bf16; f32 rtol 1e-4 / atol 1e-5).
h0 is handed over in the activation type's numbers (a carried h always is: h_last holds values of that type)."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

import ds2_oracle as DO
import ds2_stream_oracle as SO

pytestmark = pytest.mark.gpu
# one and two batch tiles, one to four k-steps, a single hand-off (T = 2) and none (T = 1)
SHAPES = [(1, 2, 32), (3, 5, 64), (17, 4, 96), (64, 3, 128), (3, 1, 64)]
ROUTES = [("persistent", torch.bfloat16), ("step", torch.float32), ("step", torch.bfloat16)]
BAR = {torch.float32: (dict(rtol=1e-4, atol=1e-5), dict(rtol=1e-4, atol=1e-5)),
       torch.bfloat16: (dict(rtol=3e-2, atol=2e-2), dict(rtol=3e-2, atol=3e-2))}


def _lengths(B, T):
    """always T, then 0 and 1 where B allows, a middle value, the rest spread over 0 .. T"""
    want = [T, 0, 1, (T + 1) // 2]
    return torch.tensor([want[b] if b < len(want) else (b * 7) % (T + 1) for b in range(B)], dtype=torch.int32)


def _case(B, T, P, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    xg = (torch.randn(B, T, 4 * P, generator=g) * 0.7).to(dtype)
    rk = (torch.randn(1, P, 4 * P, generator=g) * (1.0 / np.sqrt(P))).to(dtype)
    h0 = (torch.rand(B, P, generator=g) * 1.6 - 0.8).to(dtype).float()  # non-zero, inside tanh's range, numbers of the activation type
    c0 = torch.randn(B, P, generator=g) * 0.9
    return xg, rk, _lengths(B, T), h0.contiguous(), c0.contiguous()


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _run(dev, xg, rk, lens, h0, c0, ws=None):
    B, T, G = xg.shape
    P = G // 4
    out = (torch.empty(B, P, dtype=torch.float32, device=dev), torch.empty(B, P, dtype=torch.float32, device=dev))
    state = None if h0 is None else (h0.to(dev), c0.to(dev))
    y, h, c = K.lstm_infer_fwd(xg.to(dev).contiguous(), rk.to(dev), lens.to(dev), ndir=1, ws=ws, state=state, state_out=out)
    torch.cuda.synchronize()
    return y, h.view(B, P), c.view(B, P)


class _Route:
    def __init__(self, route):
        self.on = 1 if route == "persistent" else 0

    def __enter__(self):
        self.prev = K.lstm_set_persist(self.on)

    def __exit__(self, *a):
        K.lstm_set_persist(self.prev)


@pytest.mark.parametrize("B,T,P", SHAPES)
@pytest.mark.parametrize("route,dtype", ROUTES)
def test_state_against_the_oracle_and_split_invariance(dev, B, T, P, route, dtype):
    xg, rk, lens, h0, c0 = _case(B, T, P, dtype, seed=3000 * B + P + T)
    with _Route(route):
        ws = torch.zeros(K.lstm_infer_workspace_size(B, T, P, 1, K._dt(xg)), dtype=torch.uint8, device=dev)
        y, h, c = _run(dev, xg, rk, lens, h0, c0, ws)
        if route == "persistent":  # {count, abort}: every workgroup arrived after every step but the last - this route ran, no wait timed out
            assert ws[:64].view(torch.int32)[:2].tolist() == [(P // 16) * (T - 1), 0]
        # ---- the float64 recurrence from the same state
        y_ref, h_ref, c_ref = SO.lstm_state(xg.double(), rk[0].double(), lens, h0, c0, hround=DO.bf16_round if dtype == torch.bfloat16 else None)
        ybar, cbar = BAR[dtype]
        np.testing.assert_allclose(y.float().cpu().numpy(), y_ref.numpy(), **ybar)
        np.testing.assert_allclose(h.cpu().numpy(), h_ref.numpy(), **ybar)
        np.testing.assert_allclose(c.cpu().numpy(), c_ref.numpy(), **cbar)
        assert float((y.float().cpu() - SO.lstm_state(xg.double(), rk[0].double(), lens)[0]).abs().max()) > 0.05 or int(lens.max()) == 0, \
            "the state changes the output: the comparison above is not one against the zero-state run"
        yc = y.cpu()
        for b in range(B):
            n = int(lens[b])
            assert not yc[b, n:].any(), b  # masked outputs are exactly zero
            if n == 0:  # an idle stream: zero rows, its state back bit for bit
                assert _same(h[b], h0[b]) and _same(c[b], c0[b]), b
        # ---- two calls, every stream split at its own point (set through lengths): call 1 walks frames [0, s_b), call 2 the rest, which
        # stands at the front of its rows as a session's next chunk does
        split = torch.tensor([(int(lens[b]) * (b % 3 + 1)) // 3 for b in range(B)], dtype=torch.int32)  # 1/3, 2/3, all of the stream
        ya, ha, ca = _run(dev, xg, rk, split, h0, c0)
        xb = torch.zeros_like(xg)
        for b in range(B):
            s, n = int(split[b]), int(lens[b])
            xb[b, :n - s] = xg[b, s:n]
        yb, hb, cb = _run(dev, xb, rk, lens - split, ha.cpu(), ca.cpu())
        assert _same(hb, h) and _same(cb, c)
        for b in range(B):
            s, n = int(split[b]), int(lens[b])
            assert _same(ya[b, :s], y[b, :s]) and _same(yb[b, :n - s], y[b, s:n]), b
            assert not ya[b, s:].any() and not yb[b, n - s:].any(), b
        # ---- T calls of one step each
        hk, ck = h0, c0
        for t in range(T):
            live = (lens > t).to(torch.int32)
            yk, hk, ck = _run(dev, xg[:, t:t + 1], rk, live, hk.cpu(), ck.cpu())
            assert _same(yk[:, 0], y[:, t]), t
        assert _same(hk, h) and _same(ck, c)


@pytest.mark.parametrize("B,T,P", SHAPES)
@pytest.mark.parametrize("route,dtype", ROUTES)
def test_zero_state_is_the_stateless_entry(dev, B, T, P, route, dtype):
    xg, rk, lens, _, _ = _case(B, T, P, dtype, seed=4000 * B + P + T)
    zero = torch.zeros(B, P)
    with _Route(route):
        y0, h0, c0 = _run(dev, xg, rk, lens, None, None)       # tfasr_lstm_infer_fwd: the state entry with both NULL
        y1, h1, c1 = _run(dev, xg, rk, lens, zero, zero.clone())  # tfasr_lstm_infer_fwd_state on a state of zeros
    assert _same(y0, y1) and _same(h0, h1) and _same(c0, c1)
    assert bool(y0.any()) or int(lens.max()) == 0


@pytest.mark.parametrize("route,dtype", ROUTES)
def test_idle_streams_get_their_state_back(dev, route, dtype):
    """every stream idle (lengths 0), B = 1 and a second batch tile: nothing but zero rows, h and c bit for bit"""
    for B, T, P in ((1, 2, 32), (17, 3, 64)):
        xg, rk, _, h0, c0 = _case(B, T, P, dtype, seed=5000 + B)
        with _Route(route):
            y, h, c = _run(dev, xg, rk, torch.zeros(B, dtype=torch.int32), h0, c0)
        assert not y.any() and _same(h, h0) and _same(c, c0)


@pytest.mark.parametrize("route,dtype", ROUTES)
def test_a_new_state_in_the_old_ones_memory_is_refused(dev, route, dtype):
    """everything else about the call is legal: the refusal is the aliasing rule's (T = 1: the launch with no hand-off between the reads of
    h0 and the writes of h_last), and nothing was launched - the buffers are as they were"""
    from tensorflowasr_amd._lib import TfasrError

    xg, rk, lens, h0, c0 = (t.to(dev) for t in _case(3, 1, 64, dtype, seed=6000))
    spare = torch.empty_like(h0)
    keep = (h0.clone(), c0.clone())
    with _Route(route):
        for out in ((h0, spare), (spare, c0), (c0, spare), (spare, h0)):
            with pytest.raises(TfasrError, match="lstm_infer_fwd_state"):
                K.lstm_infer_fwd(xg, rk, lens, ndir=1, state=(h0, c0), state_out=out)
        with pytest.raises(TfasrError, match="lstm_infer_fwd_state"):  # a state cannot continue a backward direction
            K.lstm_infer_fwd(torch.cat([xg, xg], 2), torch.cat([rk, rk]), lens, ndir=2, state=(h0, c0),
                             state_out=(torch.empty(2, 3, 64, device=dev), torch.empty(2, 3, 64, device=dev)))
    torch.cuda.synchronize()
    assert torch.equal(h0, keep[0]) and torch.equal(c0, keep[1])
