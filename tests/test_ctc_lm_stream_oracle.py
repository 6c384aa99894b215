"""tests/ctc_lm_stream_oracle.py pinned on the CPU: without a horizon its final n-best is ctc_lm_oracle.fused_beam_search's for every
chunk size (a prune point that prunes nothing changes nothing); at zero weights, with every class listed, its steps are
beam_horizon_oracle.ctc_stream's; and the inputs of the GPU rule test (test_ctc_lm_stream_gpu.py) have the margins and the events
that test needs."""
import numpy as np
import pytest

import beam_horizon_oracle as HO
import ctc_lm_oracle as O
import ctc_lm_stream_oracle as SO


@pytest.mark.parametrize("V,W", [(5, 1), (5, 3), (12, 2), (29, 4)])
def test_without_a_horizon_the_final_nbest_is_the_one_shot_search(V, W):
    rng = np.random.default_rng(V + W)
    T = 17
    for blank in (0, V - 1):
        for order, (alpha, beta) in ((1, (0.5, 0.0)), (3, (1.2, -0.6)), (5, (0.3, 0.9))):
            lm = O.markov_lm(V, blank, order, seed=order)
            x = (rng.standard_normal((T, V)) * 2.5).astype(np.float32)
            want = O.fused_beam_search(x, T, W, blank, lm, alpha, beta)
            for C in (1, 3, 7, T):
                r = SO.ctc_lm_stream(x, W, blank, C, lm, alpha, beta)
                assert [y for y, *_ in r["final"]] == [y for y, *_ in want], (V, W, blank, order, C)
                np.testing.assert_array_equal(np.array([v[1:] for v in r["final"]]), np.array([v[1:] for v in want]))
                assert r["steps"][-1][0] == T and len(r["steps"]) == -(-T // C)
                for (_, committed, live), parts in zip(r["steps"], r["parts"]):
                    assert all(y[:len(committed)] == committed for y, _ in live)  # the plain commit: the common prefix
                    assert [s for _, s in live] == [a + l for a, l in parts]


@pytest.mark.parametrize("W", [2, 4, 8])
def test_at_zero_weights_the_steps_are_the_plain_streams(W):
    V, blank, T = 5, 4, 60  # V - 1 <= 2W: every class is listed, the fused frame rule is the plain one
    lm = O.markov_lm(V, blank, 3, seed=3)
    for seed in (1, 6, 13):
        x = HO.quiet_loud(np.random.default_rng(seed), T, V, blank)
        for H in (None, 4, 16):
            for C in (1, 4):
                for Tcap in (None, 24):
                    a = SO.ctc_lm_stream(x, W, blank, C, lm, 0.0, 0.0, H=H, Tcap=Tcap)
                    b = HO.ctc_stream(x, W, blank, C, H, Tcap)
                    assert a["steps"] == b["steps"], (W, seed, H, C, Tcap)
                    assert a["flips"] == 0 and all(l == 0.0 for p in a["parts"] for _, l in p)
                    assert (a["horizon"].fired, a["horizon"].plain) == (b["horizon"].fired, b["horizon"].plain)


def test_the_end_of_sentence_term_ranks_only_the_final_order():
    """a prune point ranks by total + lm; the final list adds the term and can order the same rows differently"""
    V, blank, W, T = 6, 5, 8, 40
    lm = O.markov_lm(V, blank, 3, seed=3)
    assert lm.has_eos
    differs = 0
    for seed in range(8):
        x = HO.quiet_loud(np.random.default_rng(seed), T, V, blank)
        r = SO.ctc_lm_stream(x, W, blank, 4, lm, 1.2, -0.6)
        running, final = [y for y, _ in r["steps"][-1][2]], [y for y, *_ in r["final"]]
        assert sorted(running) == sorted(final)
        for y, score, ac, ls in r["final"]:
            assert abs(ls - (O.lm_of(lm, 1.2, -0.6, y) + O.eos_of(lm, 1.2, y))) < 1e-9 and score == ac + ls
        differs += running != final
    assert differs > 0


def test_the_rule_tests_inputs():
    worst = {s: np.inf for s in SO.RULE_SEEDS}
    for case in SO.RULE_CASES:
        runs = SO.rule_runs(*case)
        for s, r in zip(SO.RULE_SEEDS, runs):
            worst[s] = min(worst[s], r["margin"])
        assert sum(r["horizon"].fired for r in runs) > 0, case      # some prune point removes a row
        assert sum(r["horizon"].plain for r in runs) > 0, case      # some prune point leaves the common ancestor in charge
        assert sum(r["flips"] for r in runs) > 0, case              # somewhere the fused-best row is not the acoustically best one
    assert min(worst.values()) >= 1e-3, worst
    # a horizon that ranks by the acoustic total commits something else on these inputs: the rule test can tell the two apart
    x, lm = SO.rule_inputs()
    plain = [HO.ctc_stream(x[b], 4, SO.RULE_BLANK, 4, 4) for b in range(len(x))]
    fused = SO.rule_runs(4, 4, 4, None)
    assert any(p["steps"][-1][1] != f["steps"][-1][1] for p, f in zip(plain, fused))
