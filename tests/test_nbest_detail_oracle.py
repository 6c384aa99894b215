"""tests/nbest_detail_oracle.py pinned by brute force: every frame labelling of T <= 6 frames over V = 4 classes is collapsed (repeats
merged, blanks dropped); those that give the labels are the alignments.  The best of them, and on an exact tie the one the rule names
(the final blank at the end, then the smallest move: read from the last frame backwards, always the largest state), must be the
oracle's, with its spans, sums and mean entropies."""
import itertools

import numpy as np
import pytest

import nbest_detail_oracle as O

V = 4


def _collapse(pi, blank):
    out, prev = [], None
    for c in pi:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def _states(pi, blank):
    """the state path of a labelling in the extended label sequence (even: blank, odd: label s // 2)"""
    s, out = (0 if pi[0] == blank else 1), []
    out.append(s)
    for t in range(1, len(pi)):
        c = pi[t]
        if c == blank:
            s += s & 1
        elif not (s & 1 and c == pi[t - 1]):
            s += 2 if s & 1 else 1
        out.append(s)
    return out


def _brute(lp, labels, blank):
    T = lp.shape[0]
    best, best_key, best_pi = -np.inf, None, None
    for pi in itertools.product(range(V), repeat=T):
        if _collapse(pi, blank) != list(labels):
            continue
        total = sum(lp[t, c] for t, c in enumerate(pi))
        key = tuple(reversed(_states(pi, blank)))
        if total > best or (total == best and total > -np.inf and key > best_key):
            best, best_key, best_pi = total, key, pi
    return best_pi, best


def _expect(lp, ent, labels, blank):
    """spans, sums and mean entropies read off the brute-force winner's labelling"""
    pi, score = _brute(lp, labels, blank)
    U = len(labels)
    start, end, acc, h = np.full(U, -1), np.full(U, -1), np.zeros(U), np.zeros(U)
    if pi is None:
        return start, end, acc, h, -np.inf
    u, prev = -1, None
    for t, c in enumerate(pi):
        if c != blank:
            if c != prev:
                u += 1
                start[u] = t
            end[u] = t + 1
            acc[u] += lp[t, c]
            h[u] += ent[t]
        prev = c
    return start, end, acc, np.where(start >= 0, h / np.maximum(end - start, 1), 0.0), score


CASES = [(T, labels, blank) for blank in (0, V - 1) for T in (1, 2, 3, 5, 6)
         for labels in ([], [1], [2, 2], [1, 2], [1, 1, 2], [2, 1, 2], [1, 2, 1])]


@pytest.mark.parametrize("blank", [0, V - 1])
def test_oracle_is_the_brute_force_best_alignment_on_random_floats(blank):
    rng = np.random.default_rng(5 + blank)
    for T, labels, bl in CASES:
        if bl != blank:
            continue
        x = rng.normal(size=(T, V)) * 2
        lse, ent = O.frame_stats(x)
        lp = x - lse[:, None]
        got = O.align_row(lp, ent, labels, blank)
        want = _expect(lp, ent, labels, blank)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (T, labels)
        np.testing.assert_allclose(got[2], want[2], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got[3], want[3], rtol=0, atol=1e-12)
        assert got[4] == want[4] or abs(got[4] - want[4]) < 1e-12, (T, labels)


@pytest.mark.parametrize("blank", [0, V - 1])
def test_tie_rule_on_dyadic_values(blank):
    """coarse dyadic values tie often: the spans must be those of the path the rule names, exactly"""
    rng = np.random.default_rng(11 + blank)
    ties = 0
    for T, labels, bl in CASES:
        if bl != blank:
            continue
        for _ in range(4):
            lp = -rng.integers(0, 5, size=(T, V)) / 4.0  # multiples of 1/4: every sum is exact, ties are exact and frequent
            ent = rng.integers(0, 9, size=T) / 8.0
            got = O.align_row(lp, ent, labels, blank)
            want = _expect(lp, ent, labels, blank)
            for g, w in zip(got[:4], want[:4]):
                assert np.array_equal(g, w), (T, labels, lp)
            assert got[4] == want[4]
            if want[4] > -np.inf and len(labels):
                n = sum(1 for pi in itertools.product(range(V), repeat=T)
                        if _collapse(pi, blank) == list(labels) and sum(lp[t, c] for t, c in enumerate(pi)) == want[4])
                ties += n > 1
    assert ties >= 10  # the rule was exercised, not only the maximum


def test_an_exact_tie_takes_the_final_blank_and_the_smallest_move():
    lp = np.zeros((4, V))  # every alignment of [1] scores 0
    start, end, acc, h, score = O.align_row(lp, np.array([1.0, 2.0, 4.0, 8.0]), [1], 0)
    # backwards from the last frame: the final blank as long as a stay is possible, the label on the first frame only
    assert (start.tolist(), end.tolist(), score) == ([0], [1], 0.0) and h.tolist() == [1.0]
    start, end, *_ = O.align_row(lp, np.zeros(4), [1, 1], 0)  # a repeated label needs the blank between: frames 0 and 2
    assert (start.tolist(), end.tolist()) == ([0, 2], [1, 3])
    start, end, *_ = O.align_row(lp, np.zeros(4), [1, 2], 0)  # distinct labels: stay (s-0) beats s-1 beats s-2
    assert (start.tolist(), end.tolist()) == ([0, 1], [1, 2])


def test_labels_that_do_not_fit_and_empty_rows():
    lp = np.zeros((3, V))
    start, end, acc, h, score = O.align_row(lp, np.zeros(3), [1, 1], 0)  # fits exactly: label, blank, label
    assert score == 0.0 and start.tolist() == [0, 2]
    start, end, acc, h, score = O.align_row(lp[:2], np.zeros(2), [1, 1], 0)  # misses by a frame
    assert score == -np.inf and start.tolist() == [-1, -1] and end.tolist() == [-1, -1] and acc.tolist() == [0, 0]
    assert O.align_row(lp[:0], np.zeros(0), [1], 0)[4] == -np.inf
    assert O.align_row(lp, np.zeros(3), [], 0)[4] == 0.0  # no labels: the all-blank path


def test_frame_stats_and_the_underflow_rule():
    x = np.array([[0.0, 0.0], [1.0, -np.inf], [3.0, 1.0], [1000.0, 0.0]])
    lse, ent = O.frame_stats(x)
    np.testing.assert_allclose(lse, [np.log(2), 1.0, 3 + np.log1p(np.exp(-2)), 1000.0], atol=1e-12)
    p = 1 / (1 + np.exp(-2))
    np.testing.assert_allclose(ent, [np.log(2), 0.0, -(p * np.log(p) + (1 - p) * np.log(1 - p)), 0.0], atol=1e-12)


def test_nbest_layout_dead_and_overlong_rows():
    rng = np.random.default_rng(3)
    logits = rng.normal(size=(2, 5, V))
    labels = np.array([[[1, 2, 0, 0, 0], [2, 0, 0, 0, 0], [1, 1, 1, 1, 0]], [[3, 0, 0, 0, 0], [1, 2, 1, 0, 0], [0, 0, 0, 0, 0]]])
    lens = np.array([[2, -1, 4], [1, 3, 0]])
    start, end, lp, h, score = O.nbest_align(logits, [5, 4], labels, lens, blank=0, U=3)
    assert start.shape == (2, 3, 3) and score.shape == (2, 3)
    for b, p in ((0, 1), (0, 2)):  # dead, longer than U
        assert score[b, p] == -np.inf and (start[b, p] == -1).all() and (end[b, p] == -1).all() and (lp[b, p] == 0).all() and (h[b, p] == 0).all()
    lse, ent = O.frame_stats(logits[1, :4])
    want = O.align_row(logits[1, :4] - lse[:, None], ent, [1, 2, 1], 0)
    assert np.array_equal(start[1, 1], want[0]) and score[1, 1] == want[4] and np.array_equal(lp[1, 1], want[2])
    assert np.isfinite(score[1, 2]) and (start[1, 2] == -1).all()
