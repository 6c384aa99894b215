"""tests/ctc_lm_oracle.py pinned against brute force: with a beam wide enough to hold every prefix, the float64 fused prefix beam
search ranks every labelling exactly as the enumeration of all alignments does, by log P_ctc + lm (+ the end-of-sentence term)."""
import numpy as np
import pytest

import ctc_lm_oracle as O


@pytest.mark.parametrize("V", [3, 4])
@pytest.mark.parametrize("order", [1, 2, 3])
def test_wide_beam_equals_enumeration(V, order):
    rng = np.random.default_rng(10 * V + order)
    for blank in (0, V - 1):
        lm = O.markov_lm(V, blank, order, seed=order)
        for T in (1, 2, 3, 4):
            for alpha, beta in ((0.8, 0.0), (1.5, -0.4), (0.3, 0.7)):
                x = (rng.standard_normal((T, V)) * 2.0).astype(np.float32)
                want = O.enumerate_fused(x, blank, lm, alpha, beta)
                got = O.fused_beam_search(x, T, 500, blank, lm, alpha, beta)
                assert [r[0] for r in got] == [r[0] for r in want], (V, order, blank, T, alpha, beta)
                for g, w in zip(got, want):
                    np.testing.assert_allclose(g[1:], w[1:], rtol=0, atol=1e-9)


def test_the_lm_changes_the_ranking():
    """not vacuous: with these weights the best fused labelling differs from the best acoustic one somewhere"""
    rng = np.random.default_rng(0)
    lm = O.markov_lm(4, 0, 2, seed=2)
    differs = 0
    for _ in range(20):
        x = rng.standard_normal((4, 4)).astype(np.float32)
        fused = O.enumerate_fused(x, 0, lm, 2.0, 0.0)[0][0]
        plain = max(O.enumerate_fused(x, 0, lm, 0.0, 0.0), key=lambda r: r[2])[0]
        differs += fused != plain
    assert differs > 0
