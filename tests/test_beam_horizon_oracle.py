"""The oracle of the commit horizon (tests/beam_horizon_oracle.py) pinned on the CPU: without a horizon it is the existing CTC oracle;
the rule on hand-made tries where the target lies below, at and above the common prefix; the committed prefix never shrinks and is a
prefix of every live row; a horizon keeps the uncommitted suffix short on the quiet / loud inputs of the GPU tests."""
import numpy as np
import pytest

import beam_horizon_oracle as HO
from ctc_lm_oracle import fused_beam_search, markov_lm


@pytest.mark.parametrize("V", [6, 29])
@pytest.mark.parametrize("W", [2, 8])
def test_without_a_horizon_it_is_the_existing_ctc_oracle(V, W):
    blank = V - 1
    lm = markov_lm(V, blank, 2)
    for seed in range(3):
        x = HO.quiet_loud(np.random.default_rng(seed), 60, V, blank)
        for C in (1, 4):
            got = HO.ctc_stream(x, W, blank, C)
            want = fused_beam_search(x, 60, W, blank, lm, 0.0, 0.0)
            rows = got["steps"][-1][2]
            assert [y for y, _ in rows] == [r[0] for r in want]
            np.testing.assert_allclose([t for _, t in rows], [r[2] for r in want], rtol=0, atol=1e-12)
            for frames, committed, live in got["steps"]:  # the plain commit: the common prefix of the live rows
                assert committed == HO.lcp([y for y, _ in live])
            assert got["horizon"].fired == 0


def _trie(frames):
    """frames: per frame the beam in rank order -> a Horizon(H = 2) fed one frame per prune point, and what each prune kept"""
    hz, kept = HO.Horizon(2), []
    for rows in frames:
        hz.grow(rows)
        kept.append(hz.prune(1, rows))
    return hz, kept


def test_target_below_the_common_prefix_removes_rows_and_commits_up_to_it():
    hz, kept = _trie([[(1,), ()], [(1,), (), (1, 2)], [(1, 2), (1,), ()]])
    # ids: () 0, (1,) 1, (1, 2) 2; points (1, 2), (2, 3), (3, 3): at frame 3 the point of frame 1 is 2 frames back, X = 2
    assert hz.points == [(1, 2), (2, 3), (3, 3)] and hz.case == ["below"]
    assert kept[:2] == [[(1,), ()], [(1,), (), (1, 2)]]  # no point old enough yet: the plain commit
    assert kept[2] == [(1, 2), (1,)] and hz.committed == (1,) and hz.fired == 1


def test_target_at_the_common_prefix_is_the_plain_commit():
    hz, kept = _trie([[(1,)], [(1, 2), (1, 3)], [(1, 2), (1, 3)]])
    assert hz.case == ["at"] and kept[2] == [(1, 2), (1, 3)] and hz.committed == (1,) and hz.fired == 0 and hz.plain == 1


def test_target_above_the_common_prefix_leaves_the_common_prefix_in_charge():
    # (1, 2) enters at frame 2, after the point of frame 1: at frame 3 it is younger than the horizon, but every live row has it
    hz, kept = _trie([[(1,)], [(1, 2)], [(1, 2, 3), (1, 2, 4)]])
    assert hz.case == ["above"] and kept[2] == [(1, 2, 3), (1, 2, 4)] and hz.committed == (1, 2) and hz.fired == 0


def test_the_best_row_decides_and_ties_in_age_do_not():
    # both branches are old enough; the best row's one wins, the other leaves with all its extensions
    frames = [[(1,), (2,)], [(1,), (2,), (2, 5)], [(2, 5), (1,), (2,)]]
    hz, kept = _trie(frames)
    assert kept[2] == [(2, 5), (2,)] and hz.committed == (2,)  # X = 3 from frame 1: (2,) has id 2, (2, 5) id 3
    hz, kept = _trie(frames + [[(2, 5), (1,), (2,), (1, 7)]])  # (had the rows of frame 3 been left in)
    assert kept[3] == [(2, 5)] and hz.committed == (2, 5)  # X = 4 from frame 2


@pytest.mark.parametrize("H", [4, 16])
@pytest.mark.parametrize("W", [2, 8])
def test_committed_prefix_grows_and_bounds_the_uncommitted_suffix(W, H):
    V, blank, T, C = 6, 5, 400, 4
    x = HO.quiet_loud(np.random.default_rng(W), T, V, blank)
    plain, hor = HO.ctc_stream(x, W, blank, C), HO.ctc_stream(x, W, blank, C, H)
    last = ()
    for frames, committed, live in hor["steps"]:  # (Horizon.prune asserts the same at every point)
        assert committed[:len(last)] == last and all(y[:len(committed)] == committed for y, _ in live)
        last = committed
    suffix = lambda run: max(max(len(y) for y, _ in live) - len(c) for _, c, live in run["steps"])
    assert hor["horizon"].fired > 0 and hor["horizon"].plain > 0
    # a label below the target is younger than the point the target was read from, which is less than H + C frames back, and a row
    # gains one label per frame at most
    assert suffix(hor) <= H + C - 1 < suffix(plain), (suffix(hor), suffix(plain))
    assert np.isfinite(hor["margin"]) and hor["margin"] >= 0.0


def _runs(seed, W, Tcap):
    x = HO.quiet_loud(np.random.default_rng(seed), 400, 6, 5)
    return [[(f, c, [y for y, _ in live]) for f, c, live in HO.ctc_stream(x, W, 5, 4, 8, Tcap=cap)["steps"]] for cap in (None, Tcap)]


def test_a_compaction_makes_a_returning_sequence_young():
    """Without a horizon a compaction is neutral: a dropped sequence that wins again gets a fresh node, and nothing reads a node's age.
    The horizon does: the fresh node counts as younger than the sequence is, so the target can stop one label earlier than in a stream
    that was never compacted, and the beams part ways.  Pinned here on the inputs of test_beam_horizon_gpu's capacity test: seed 40 at
    W = 8 differs from frame 260 on (57 against 58 labels committed), seeds 41 and 43 do not, and W = 2 never does on these."""
    plain, compacted = _runs(40, 8, 32)
    first = next(i for i, (p, q) in enumerate(zip(plain, compacted)) if p != q)
    assert plain[first][0] == 260 and (len(plain[first][1]), len(compacted[first][1])) == (58, 57)
    assert compacted[first][1] == plain[first][1][:57]  # the compacted stream commits later, not differently
    for seed, W in ((41, 8), (43, 8), (40, 2), (41, 2)):
        plain, compacted = _runs(seed, W, 32)
        assert plain == compacted, (seed, W)
