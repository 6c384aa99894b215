"""tfasr_ctc_beam_search_lm: the device prefix beam search with an n-gram LM fused in decodes exactly like the host routine
tfasr_ctc_beam_search_lm_host (tokens, lengths and lm_score bit for bit), changes nothing at zero weights (bit for bit against
tfasr_ctc_beam_search), keeps one trie node per label sequence, keeps the exact-tie order, returns the exact n-best list when the
beam holds every prefix, accepts bf16 logits, is deterministic at the bench shape, and refuses a beam wider than 32."""
import numpy as np
import pytest
import torch

import ctc_lm_oracle as O
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.lm import NGramLM

pytestmark = pytest.mark.gpu

WEIGHTS = ((0.5, 0.0), (1.2, -0.6), (0.3, 0.9))


def device_lm(x, lens, tables, beam, blank, top_paths=1, dtype=torch.float32):
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda", dtype)
    out = K.ctc_beam_search_lm(xt, torch.tensor(lens, dtype=torch.int32), tables, beam_width=beam, top_paths=top_paths, blank_index=blank)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def assert_same_as_host(x, lens, tables, beam, blank, top_paths=1, lp_tol=1e-4, what=""):
    h = O.host_lm(x, lens, tables, beam, blank, top_paths)
    d = device_lm(x, lens, tables, beam, blank, top_paths)
    np.testing.assert_array_equal(d[1], h[1], err_msg=what)                      # lengths
    np.testing.assert_array_equal(d[0], h[0], err_msg=what)                      # tokens
    np.testing.assert_array_equal(d[4], h[4], err_msg=what)                      # lm_score, exactly
    np.testing.assert_allclose(d[3], h[3], rtol=0, atol=lp_tol, err_msg=what)    # log_prob
    np.testing.assert_array_equal(d[2], (d[3] + d[4]).astype(np.float32), err_msg=what)  # score = one float32 add
    return d


@pytest.mark.parametrize("V", [5, 29, 1000])
def test_parity_with_the_host_routine(dev, V):
    rng = np.random.default_rng(V)
    B, T = 8, 60
    lens = [60, 0, 1, 37, 60, 12, 59, 2]
    case = 0
    for beam in (1, 2, 4, 10, 16, 32):
        for blank in (0, V - 1):
            order = (1, 3, 5)[case % 3]
            alpha, beta = WEIGHTS[(case // 3) % 3]
            case += 1
            tables = O.markov_lm(V, blank, order, seed=order).tables(alpha, beta)
            x = (rng.standard_normal((B, T, V)) * (2.0, 3.0, 4.0)[beam % 3]).astype(np.float32)
            assert_same_as_host(x, lens, tables, beam, blank, top_paths=min(beam, 3),
                                what=f"V={V} beam={beam} blank={blank} order={order} alpha={alpha} beta={beta}")


@pytest.mark.parametrize("V", [29, 1000])
def test_zero_weights_change_nothing_bit_for_bit(dev, V):
    rng = np.random.default_rng(50 + V)
    B, T = 8, 60
    lens = [60, 0, 1, 37, 60, 12, 59, 2]
    for beam in (1, 4, 10, 32):
        for blank in (0, V - 1):
            tables = O.markov_lm(V, blank, 3, seed=3).tables(0.0, 0.0)
            x = (rng.standard_normal((B, T, V)) * 3.0).astype(np.float32)
            P = min(beam, 4)
            toks, n, score, lp, ls = device_lm(x, lens, tables, beam, blank, top_paths=P)
            ut, un, ulp = K.ctc_beam_search_device(torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32), beam_width=beam,
                                                   top_paths=P, blank_index=blank)
            np.testing.assert_array_equal(toks, ut.cpu().numpy())
            np.testing.assert_array_equal(n, un.cpu().numpy())
            np.testing.assert_array_equal(lp.view(np.int32), ulp.cpu().numpy().view(np.int32))
            assert not ls.any()


def test_prefix_reentry_small_alphabet_narrow_beam(dev):
    """a prefix that leaves the beam and comes back while one of its extensions stayed keeps ONE node (its mass merges, its lm is kept)"""
    rng = np.random.default_rng(5)
    tables = O.markov_lm(3, 0, 3, seed=2).tables(0.7, 0.2)
    for beam in (2, 3):
        x = (rng.standard_normal((300, 14, 3)) * 1.5).astype(np.float32)
        assert_same_as_host(x, [14] * 300, tables, beam, 0, top_paths=beam, what=f"beam={beam}")


def test_exact_ties_follow_label_sequence_order(dev):
    rng = np.random.default_rng(11)
    # duplicated columns: classes 1 and 3 (and 2 and 4) always score the same, and the LM saw them used identically
    base = (rng.standard_normal((6, 20, 3)) * 2.0).astype(np.float32)
    dup = np.concatenate([base, base[:, :, 1:3], np.full((6, 20, 1), -1.0, np.float32)], axis=2)  # V = 6, blank 5 or 0
    twin = {1: 3, 2: 4, 3: 1, 4: 2}
    seqs = [[int(t) for t in rng.integers(1, 5, size=rng.integers(1, 7))] for _ in range(40)]
    seqs += [[twin[t] for t in s] for s in seqs]  # every sequence and its mirror image: twins get identical statistics
    for blank in (5, 0):
        lm = NGramLM.estimate(seqs, 2, 6, blank)
        for a, b in ((1, 3), (2, 4)):
            assert lm.log_prob([], a) == lm.log_prob([], b) and lm.log_prob([a], b) == lm.log_prob([b], a)
        tables = lm.tables(0.8, -0.3)
        for beam in (1, 2, 4, 10):
            assert_same_as_host(dup, [20, 19, 7, 1, 20, 3], tables, beam, blank, top_paths=beam, what=f"dup beam={beam} blank={blank}")
    # all-equal rows under a unigram model that scores every token alike: every candidate of a frame ties with its siblings
    flat = np.zeros((4, 9, 4), np.float32)
    flat[1] = 0.5
    flat[2, :, :] = rng.standard_normal((9, 1)).astype(np.float32)
    for blank in (0, 3):
        toks = [t for t in range(4) if t != blank]
        lm = NGramLM.estimate([[t] for t in toks], 1, 4, blank)
        tables = lm.tables(1.0, 0.5)
        for beam in (1, 3, 8, 16):
            assert_same_as_host(flat, [9, 8, 5, 2], tables, beam, blank, top_paths=beam, what=f"flat beam={beam} blank={blank}")


def test_nbest_exact_with_a_wide_beam(dev):
    rng = np.random.default_rng(3)
    B, T, V, W = 6, 4, 3, 32
    lens = [4, 3, 4, 2, 4, 1]
    for blank in (0, 2):
        for order in (1, 2, 3):
            lm = O.markov_lm(V, blank, order, seed=order)
            alpha, beta = WEIGHTS[order % 3]
            x = (rng.standard_normal((B, T, V)) * 2.0).astype(np.float32)
            toks, n, score, lp, ls = assert_same_as_host(x, lens, lm.tables(alpha, beta), W, blank, top_paths=W)
            for b, Tb in enumerate(lens):
                want = O.enumerate_fused(x[b, :Tb], blank, lm, alpha, beta)
                for p in range(W):
                    if p < len(want):
                        lab, wscore, wlp, wls = want[p]
                        assert toks[b, p, :n[b, p]].tolist() == list(lab), (blank, order, b, p)
                        assert not toks[b, p, n[b, p]:].any()
                        assert abs(lp[b, p] - wlp) < 1e-5, (blank, order, b, p, lp[b, p], wlp)
                    else:  # fewer labellings than paths: empty, length 0
                        assert n[b, p] == 0 and not toks[b, p].any() and lp[b, p] == -np.inf and score[b, p] == -np.inf


def test_bf16_logits_decode_like_their_f32_upcast(dev):
    rng = np.random.default_rng(8)
    x = torch.from_numpy((rng.standard_normal((8, 40, 29)) * 3.0).astype(np.float32)).to(torch.bfloat16)
    x32 = x.float().numpy()
    lens = [40, 33, 1, 0, 40, 17, 28, 39]
    tables = O.markov_lm(29, 0, 3, seed=3).tables(0.6, 0.1)
    for beam in (1, 4, 10):
        a = device_lm(x32, lens, tables, beam, 0, top_paths=min(beam, 3), dtype=torch.bfloat16)
        b = device_lm(x32, lens, tables, beam, 0, top_paths=min(beam, 3), dtype=torch.float32)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)


def test_deterministic_at_the_bench_shape(dev):
    rng = np.random.default_rng(1)
    B, T, V, W = 32, 250, 1000, 10
    x = torch.from_numpy((rng.standard_normal((B, T, V)) * 3.0).astype(np.float32)).cuda()
    lens = torch.tensor(rng.integers(200, T + 1, size=B), dtype=torch.int32)
    tables = O.markov_lm(V, 0, 3, seed=3).tables(0.5, 0.1)
    a = [o.clone() for o in K.ctc_beam_search_lm(x, lens, tables, beam_width=W, top_paths=4, blank_index=0)]
    b = K.ctc_beam_search_lm(x, lens, tables, beam_width=W, top_paths=4, blank_index=0)
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert int(a[1].max()) > 0 and bool(torch.isfinite(a[2]).all())


def test_a_beam_wider_than_32_is_refused(dev):
    tables = O.markov_lm(29, 0, 3, seed=3).tables(0.5, 0.0)
    with pytest.raises(ValueError, match="32"):
        K.ctc_beam_search_lm(torch.zeros(2, 10, 29, device="cuda"), torch.tensor([10, 3], dtype=torch.int32), tables, beam_width=33)
