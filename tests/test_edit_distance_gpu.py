"""The edit-distance kernels (csrc/edit_distance.hip) against metrics.edit_distance_host, which tests/test_metrics.py pins to an
enumeration of all alignments.  All five outputs are integers and must be equal.

Tiers: one wave per pair with 1 / 2 / 4 / 8 reference columns per lane (M <= 64 / 128 / 256 / 512), then one workgroup per pair with 4
columns per thread (M <= 4096); the widths below sit on both sides of every one of those limits and of the 64-entry chunks of the
load phase."""
import ctypes

import numpy as np
import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import metrics as M

pytestmark = pytest.mark.gpu
I32 = torch.int32
WIDTHS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1025, 4096]
ALPHABETS = (2, 4, 1000)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


def table(counts):
    return np.stack([np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c) for c in counts], 1)


def ragged(rng, per_alphabet, width):
    """8 rows per alphabet: lengths anywhere in 0 .. width with 0 and the full width present; past its length a row holds -7 (even
    rows) or in-alphabet symbols (odd rows)"""
    rows, lens = [], []
    for a in ALPHABETS:
        x = rng.integers(0, a, (per_alphabet, width)).astype(np.int32)
        n = rng.integers(0, width + 1, per_alphabet).astype(np.int32)
        n[0], n[1] = 0, width
        for k in range(0, per_alphabet, 2):
            x[k, n[k]:] = -7
        rows.append(x)
        lens.append(n)
    return np.concatenate(rows), np.concatenate(lens)


def on_device(dev, hyp, ref, hyp_len=None, ref_len=None, skip_id=-1):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return K.edit_distance(t(hyp), t(ref), t(hyp_len), t(ref_len), skip_id).cpu().numpy()


@pytest.mark.parametrize("Mw", WIDTHS)
def test_widths_across_lane_column_and_tier_boundaries(dev, Mw):
    rng = np.random.default_rng(1000 + Mw)
    ref, ref_len = ragged(rng, 8, Mw)
    for Nw in sorted({min(max(n, 0), 4096) for n in (0, 1, Mw - 1, Mw, Mw + 1, 2 * Mw)}):
        hyp, hyp_len = ragged(rng, 8, Nw)
        if Nw == Mw and Mw > 0:  # near-identical pairs: long runs of hits, a few edits
            hyp[2::2] = ref[2::2]
            hyp_len[2::2] = ref_len[2::2]
            hyp[2::2, Mw // 2] += 1
        want = table(M.edit_distance_host(hyp, ref, hyp_len, ref_len))
        got = on_device(dev, hyp, ref, hyp_len, ref_len)
        np.testing.assert_array_equal(got, want, err_msg=f"M {Mw} N {Nw}")
        assert (got[:, 1] + got[:, 2] + got[:, 3] == ref_len).all() and (got[:, 1] + got[:, 2] + got[:, 4] == hyp_len).all()


def test_tie_rule_pins_identical_disjoint_and_empty_rows(dev):
    hyp = np.array([[0, 1, 9], [7, 7, 7], [1, 7, 7], [3, 4, 5], [3, 4, 5], [9, 9, 9]], np.int32)
    ref = np.array([[1, 0, 9], [1, 2, 9], [8, 8, 8], [3, 4, 5], [6, 7, 8], [9, 9, 9]], np.int32)
    hyp_len = np.array([2, 0, 1, 3, 3, 0], np.int32)
    ref_len = np.array([2, 2, 0, 3, 3, 0], np.int32)
    got = on_device(dev, hyp, ref, hyp_len, ref_len)
    assert got.tolist() == [[2, 1, 0, 1, 1], [2, 0, 0, 2, 0], [1, 0, 0, 0, 1], [0, 3, 0, 0, 0], [3, 0, 3, 0, 0], [0, 0, 0, 0, 0]]
    np.testing.assert_array_equal(got, table(M.edit_distance_host(hyp, ref, hyp_len, ref_len)))


@pytest.mark.parametrize("Nw, Mw", [(150, 70), (64, 64), (700, 600)])
def test_compaction_mode(dev, Nw, Mw):
    """rows with the skip id and -1 scattered through them score like the explicit-length call on the rows compacted beforehand"""
    rng = np.random.default_rng(Nw)
    P, skip = 12, 0

    def scattered(width):
        x = rng.integers(1, 6, (P, width)).astype(np.int32)
        drop = rng.random((P, width)) < rng.random((P, 1))
        x[drop] = np.where(rng.random(int(drop.sum())) < 0.5, skip, -1)
        x[0] = skip  # an all-blank row: length 0
        x[1] = rng.integers(1, 6, width)  # nothing to drop: the full width
        packed = np.full((P, width), -7, np.int32)
        n = np.zeros(P, np.int32)
        for p in range(P):
            keep = x[p][(x[p] >= 0) & (x[p] != skip)]
            packed[p, : len(keep)], n[p] = keep, len(keep)
        return x, packed, n

    hyp, hyp_packed, hyp_len = scattered(Nw)
    ref, ref_packed, ref_len = scattered(Mw)
    assert hyp_len[0] == 0 and hyp_len[1] == Nw
    want = on_device(dev, hyp_packed, ref_packed, hyp_len, ref_len)
    np.testing.assert_array_equal(want, table(M.edit_distance_host(hyp_packed, ref_packed, hyp_len, ref_len)))
    np.testing.assert_array_equal(on_device(dev, hyp, ref, None, None, skip), want)          # both sides
    np.testing.assert_array_equal(on_device(dev, hyp, ref_packed, None, ref_len, skip), want)  # the hypotheses only (evaluate's call)
    np.testing.assert_array_equal(on_device(dev, hyp_packed, ref, hyp_len, None, skip), want)  # the references only
    np.testing.assert_array_equal(table(M.edit_distance_host(hyp, ref, skip_id=skip)), want)
    np.testing.assert_array_equal(table(M.edit_distance(torch.from_numpy(hyp).to(dev), torch.from_numpy(ref).to(dev), skip_id=skip)), want)


@pytest.mark.parametrize("P", [1, 33, 1000])
def test_pair_counts(dev, P):
    rng = np.random.default_rng(P)
    hyp, ref = rng.integers(0, 4, (P, 37)).astype(np.int32), rng.integers(0, 4, (P, 40)).astype(np.int32)
    hyp_len, ref_len = rng.integers(0, 38, P).astype(np.int32), rng.integers(0, 41, P).astype(np.int32)
    np.testing.assert_array_equal(on_device(dev, hyp, ref, hyp_len, ref_len), table(M.edit_distance_host(hyp, ref, hyp_len, ref_len)))


def test_non_default_stream(dev):
    rng = np.random.default_rng(5)
    hyp, ref = rng.integers(0, 4, (16, 90)).astype(np.int32), rng.integers(0, 4, (16, 100)).astype(np.int32)
    hyp_len, ref_len = rng.integers(0, 91, 16).astype(np.int32), rng.integers(0, 101, 16).astype(np.int32)
    want = on_device(dev, hyp, ref, hyp_len, ref_len)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        got = on_device(dev, hyp, ref, hyp_len, ref_len)
    stream.synchronize()
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("Nw, Mw", [(50, 40), (300, 700)])
def test_nothing_is_written_past_the_outputs(dev, Nw, Mw):
    """a patterned guard region behind `counts` and behind the workspace is intact after the call (one case per kernel)"""
    rng = np.random.default_rng(7)
    P, GUARD, PAT = 9, 4096, 0x5A
    hyp, ref = rng.integers(0, 4, (P, Nw)).astype(np.int32), rng.integers(0, 4, (P, Mw)).astype(np.int32)
    hyp_len, ref_len = rng.integers(0, Nw + 1, P).astype(np.int32), rng.integers(0, Mw + 1, P).astype(np.int32)
    need = K.edit_distance_workspace_size(P, Nw, Mw)
    out = torch.full((P * 5 * 4 + GUARD,), PAT, dtype=torch.uint8, device=dev)
    ws = torch.full((need + GUARD,), PAT, dtype=torch.uint8, device=dev)
    d = [torch.from_numpy(a).to(dev) for a in (hyp, hyp_len, ref, ref_len)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = _lib.load().tfasr_edit_distance(p(d[0]), p(d[1]), p(d[2]), p(d[3]), P, Nw, Mw, -1, p(out), p(ws), need, K._stream())
    torch.cuda.synchronize()
    assert st == 0
    assert bool((out[P * 5 * 4:] == PAT).all()) and bool((ws[need:] == PAT).all())
    got = out[: P * 5 * 4].view(I32).view(P, 5).cpu().numpy()
    np.testing.assert_array_equal(got, table(M.edit_distance_host(hyp, ref, hyp_len, ref_len)))
