"""CPU: pin tests/decode_oracle.py (the stage-by-stage search step the GPU tests of csrc/decode_step.hip compare against) to the search
loops of oracle/conformer_ref.py, which the reference pins (tests/test_reference_pins.py) hold to the reference itself."""
import numpy as np
import torch

from oracle import conformer_ref as R

import decode_oracle as DO

B, T = 5, 9
LENS = [9, 4, 7, 1, 6]


def _case(seed=12, blank_bias=0.0, sharpen=4.0):
    """tiny oracle weights with nonzero biases; a sharpened vocabulary projection so rows emit a mix of blanks and symbols"""
    W = R.init_weights(R.conformer_config("tiny"), seed=seed, scale_bias=0.1)
    W["joint/vocab/w"] = W["joint/vocab/w"] * sharpen
    W["joint/vocab/b"] = W["joint/vocab/b"].clone()
    W["joint/vocab/b"][0] += blank_bias
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(B, T, W["joint/enc/w"].shape[0], generator=g) * 2
    # the joint's encoder projection frame by frame, the shape the reference loop multiplies ([B, 1, d] @ [d, J])
    encj = torch.cat([enc[:, t:t + 1] @ W["joint/enc/w"] + W["joint/enc/b"] for t in range(T)], 1)
    return W, enc, encj


def test_step_and_update_reproduce_recognize_batch_exactly():
    seen = set()
    for bias in (0.0, 2.0, 4.0):
        W, enc, encj = _case(blank_bias=bias)
        tok, prev, h, c = R.recognize_batch(enc, LENS, W)
        st = DO.search(0, W, encj, LENS, dtype=torch.float32)
        np.testing.assert_array_equal(st["tokens"], tok.numpy())
        np.testing.assert_array_equal(st["prev_tok"], prev.numpy().reshape(-1))
        np.testing.assert_array_equal(st["h"], h.numpy())
        np.testing.assert_array_equal(st["c"], c.numpy())
        seen.update(int((row[2:] != 0).sum()) for row in st["tokens"])
    assert 0 in seen and max(seen) == 2 * T - 1 and len(seen) >= 3  # rows that emit nothing, rows that fill the buffer, and a mix between


def test_step_and_update_reproduce_recognize_single_exactly():
    emitted = []
    for bias in (0.0, 2.0, 4.0):
        W, enc, encj = _case(blank_bias=bias)
        for b, n in enumerate(LENS):
            tok, prev, h, c = R.recognize_single(enc[b:b + 1, :n], [n], W)
            st = DO.search(1, W, encj[b:b + 1, :n], [n], dtype=torch.float32)
            np.testing.assert_array_equal(st["tokens"], tok.numpy())
            np.testing.assert_array_equal(st["prev_tok"], prev.numpy().reshape(-1))
            np.testing.assert_array_equal(st["h"], h.numpy())
            np.testing.assert_array_equal(st["c"], c.numpy())
            assert st["frame_idx"][0] == n
            emitted.append(int(st["tok_idx"][0]) + 1)
    assert min(emitted) == 0 and max(emitted) == 3 * T  # nothing but blanks, and three symbols on every frame


def test_mode_2_is_mode_1_on_every_row_alone():
    for bias in (0.0, 2.0, 4.0):
        W, _, encj = _case(blank_bias=bias)
        st2 = DO.search(2, W, encj, LENS, max_tokens=3 * T)
        for b, n in enumerate(LENS):
            st1 = DO.search(1, W, encj[b:b + 1, :n], [n])
            np.testing.assert_array_equal(st2["tokens"][b, :3 * n], st1["tokens"][0])
            assert (st2["tokens"][b, 3 * n:] == 0).all()
            for k in ("prev_tok", "tok_idx", "frame_idx"):
                assert st2[k][b] == st1[k][0], k
            # (a product of five rows and of one row may round differently: float64, to its last digits)
            np.testing.assert_allclose(st2["h"][b], st1["h"][0], rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(st2["c"][b], st1["c"][0], rtol=1e-12, atol=1e-15)
        assert (st2["per_frame"] == 0).all()


def test_float64_step_agrees_with_float32_and_stages_can_be_fed():
    W, _, encj = _case()
    g = torch.Generator().manual_seed(5)
    P = W["pred/lstm/rk"].shape[0]
    h, c = torch.randn(B, P, generator=g) * 0.5, torch.randn(B, P, generator=g) * 0.5
    prev = torch.tensor([0, 28, 3, 7, 1])
    fi = [8, 4, 5, 0, 2]  # row 1 sits one past its last frame: it reads frame nframes - 1
    a = DO.step(W, prev, h, c, encj, LENS, fi, T)
    b = DO.step(W, prev, h, c, encj, LENS, fi, T, dtype=torch.float32)
    for x, y in zip(a, b):
        assert x.dtype == torch.float64 and y.dtype == torch.float32
        np.testing.assert_allclose(y.numpy(), x.numpy(), rtol=1e-5, atol=1e-6)
    want = torch.tanh(encj[1, 3].double() + (torch.nn.functional.layer_norm(a[1][1], (P,), W["pred/ln/g"].double(), W["pred/ln/b"].double(), 1e-3)
                                             @ W["joint/pred/w"].double() + W["joint/pred/b"].double()))
    np.testing.assert_allclose(a[2][1].numpy(), want.numpy(), rtol=1e-12)
    # a later stage fed an earlier one: the earlier stages' own results are returned unchanged
    h_in, z_in = torch.randn(B, P, generator=g).double(), torch.rand(B, a[2].shape[1], generator=g).double()
    f = DO.step(W, prev, h, c, encj, LENS, fi, T, h_new=h_in, z=z_in)
    assert torch.equal(f[0], a[0]) and torch.equal(f[1], a[1])
    assert not torch.equal(f[2], a[2])
    np.testing.assert_allclose(f[3].numpy(), (z_in @ W["joint/vocab/w"].double() + W["joint/vocab/b"].double()).numpy(), rtol=1e-12)
    nol = DO.step(W, prev, h, c, encj, LENS, fi, T, ln=False)
    np.testing.assert_allclose(nol[2].numpy(), torch.tanh(encj[torch.arange(B), DO.frame_of(LENS, fi, T)].double()
                                                          + a[1] @ W["joint/pred/w"].double() + W["joint/pred/b"].double()).numpy(), rtol=1e-12)


def test_loop_condition():
    assert DO.active(0, [5, 3], [3, 2], [1, 1], 11) and not DO.active(0, [5, 3], [4, 2], [1, 1], 11)
    assert DO.active(0, [5, 3], [0, 0], [10, 9], 11) and not DO.active(0, [5, 3], [0, 0], [10, 10], 11)
    assert DO.active(2, [5, 3], [5, 2], [99, 99], 11) and not DO.active(2, [5, 3], [5, 3], [0, 0], 11)
    assert DO.active(1, [5], [4], [-1], 15) and not DO.active(1, [5], [5], [-1], 15)
