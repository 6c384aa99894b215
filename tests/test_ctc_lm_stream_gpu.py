"""The fused CTC prefix beam search in pieces (K.CtcLmBeamStream: tfasr_ctc_beam_lm_reset / _advance / _commit / _commit_horizon /
_compact / _nbest): chunking changes nothing (bit for bit against the one-shot tfasr_ctc_beam_search_lm, and against the host
routine), streams are independent, zero weights give the plain stream, a prefix re-enters across a chunk boundary, the commits follow
the LM-ranked best row, a compaction moves the per-node LM payload, and the horizon rule under fusion against the float64 oracle
(tests/ctc_lm_stream_oracle.py)."""
import numpy as np
import pytest
import torch

import beam_horizon_oracle as HO
import ctc_lm_oracle as O
import ctc_lm_stream_oracle as SO
from tensorflowasr_amd import kernels as K
from test_beam_horizon_gpu import _against_oracle, full_beam, take
from test_stream_beam_gpu import chunk_of, plan, rows_of

pytestmark = pytest.mark.gpu

WEIGHTS = ((0.5, 0.0), (1.2, -0.6), (0.3, 0.9))
B8, T60 = 8, 60
LENS = [60, 0, 1, 37, 60, 12, 59, 2]
NAMES = ("tokens", "lengths", "score", "log_prob", "lm_score")


def bits(t):
    a = t.cpu().numpy()
    return a.view(np.int32) if a.dtype == np.float32 else a


def assert_bit_equal(have, want, what):
    for name, a, b in zip(NAMES, have, want):
        a, b = bits(a), bits(b)
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=f"{what} {name}")


def one_shot(x, lens, tables, W, blank, P=None):
    return K.ctc_beam_search_lm(x, torch.tensor(lens, dtype=torch.int32), tables, beam_width=W, top_paths=P or W, blank_index=blank)


def feed(stream, x, lens, C):
    for start, nv in plan(lens, C):
        stream.advance(chunk_of(x, start, nv, C), nv)
    assert stream.frames == list(lens)


def cases(V, widths):
    """the (W, blank, order, weights, logits) of test_ctc_lm_beam_gpu.test_parity_with_the_host_routine's walk, at these widths"""
    rng = np.random.default_rng(V)
    case = 0
    for W in widths:
        for blank in (0, V - 1):
            order = (1, 3, 5)[case % 3]
            alpha, beta = WEIGHTS[(case // 3) % 3]
            case += 1
            x = (rng.standard_normal((B8, T60, V)) * (2.0, 3.0, 4.0)[W % 3]).astype(np.float32)
            yield W, blank, order, (alpha, beta), x


# ------------------------------------------------------------------------------------------------------------------ 1: chunking changes nothing
@pytest.mark.parametrize("V", [5, 29, 1000])
def test_chunking_changes_nothing(dev, V):
    for W, blank, order, (alpha, beta), x in cases(V, (1, 4, 10, 32)):
        what = f"V={V} W={W} blank={blank} order={order} alpha={alpha} beta={beta}"
        tables = O.markov_lm(V, blank, order, seed=order).tables(alpha, beta)
        xd = torch.from_numpy(x).to(dev)
        want = one_shot(xd, LENS, tables, W, blank)
        host = O.host_lm(x, LENS, tables, W, blank, top_paths=W)
        for i in (0, 1, 4):  # tokens, lengths, lm_score of the host routine, exactly
            np.testing.assert_array_equal(want[i].cpu().numpy(), host[i], err_msg=f"{what} host {NAMES[i]}")
        for C in (1, 7, 60):
            s = K.CtcLmBeamStream(B8, C, T60, V, W, tables, blank_index=blank, device=dev)
            feed(s, xd, LENS, C)
            assert_bit_equal(s.nbest(final_rows=range(B8)), want, f"{what} C={C}")
        # a stream that is still running ranks without the end-of-sentence term: lm_score = lm, score = one float32 add
        tk, n, score, lp, ls = [t.cpu().numpy() for t in s.nbest()]
        np.testing.assert_array_equal(score, (lp + ls).astype(np.float32))
        for b in range(B8):
            for p in range(W):
                if lp[b, p] != -np.inf:
                    st, acc = tables.start, np.float32(0.0)
                    for c in tk[b, p, :n[b, p]]:
                        inc, st = O.NGramLM.walk(tables, st, int(c))
                        acc = np.float32(acc + inc)
                    assert ls[b, p] == acc, (what, b, p)


def test_bf16_logits_stream_like_the_one_shot_search(dev):
    rng = np.random.default_rng(8)
    V, W, blank = 29, 4, 0
    x = torch.from_numpy((rng.standard_normal((B8, T60, V)) * 3.0).astype(np.float32)).to(dev).to(torch.bfloat16)
    tables = O.markov_lm(V, blank, 3, seed=3).tables(0.6, 0.1)
    want = one_shot(x, LENS, tables, W, blank)
    assert_bit_equal(want, one_shot(x.float(), LENS, tables, W, blank), "bf16 against its f32 upcast")
    for C in (1, 7):
        s = K.CtcLmBeamStream(B8, C, T60, V, W, tables, blank_index=blank, device=dev)
        feed(s, x, LENS, C)
        assert_bit_equal(s.nbest(final_rows=range(B8)), want, f"bf16 C={C}")


# ------------------------------------------------------------------------------------------------------------------ 2: stream independence
def test_a_reset_stream_leaves_the_others_bit_identical(dev):
    V, W, blank, C = 29, 4, 0, 7
    rng = np.random.default_rng(21)
    x = torch.from_numpy((rng.standard_normal((B8, T60, V)) * 3.0).astype(np.float32)).to(dev)
    y = torch.from_numpy((rng.standard_normal((1, 23, V)) * 3.0).astype(np.float32)).to(dev)  # the utterance that takes slot 3
    tables = O.markov_lm(V, blank, 3, seed=3).tables(1.2, -0.6)
    want = [t.cpu() for t in one_shot(x, LENS, tables, W, blank)]
    other = [t.cpu() for t in one_shot(y, [23], tables, W, blank)]
    s = K.CtcLmBeamStream(B8, C, T60, V, W, tables, blank_index=blank, device=dev)
    steps = plan(LENS, C)
    half = len(steps) // 2
    for start, nv in steps[:half]:
        s.advance(chunk_of(x, start, nv, C), nv)
    assert 0 < s.frames[3] < LENS[3]
    before = [t.clone() for t in s.nbest(final_rows=range(B8))]
    s.reset(rows=[3])
    after = s.nbest(final_rows=range(B8))
    for name, p, q in zip(NAMES, before, after):
        for b in range(B8):
            if b != 3:
                assert torch.equal(p[b], q[b]), (name, b)
    assert rows_of(*after[:3])[3] == [()] and float(after[4][3, 0]) == float(before[4][1, 0])  # the empty row: the term from `start`
    pos = 0
    for start, nv in steps[half:]:
        xc = chunk_of(x, start, nv, C)
        nv = list(nv)
        nv[3] = min(C, 23 - pos)
        xc[3] = 1e4
        xc[3, :nv[3]] = y[0, pos:pos + nv[3]]
        pos += nv[3]
        s.advance(xc, nv)
    assert pos == 23
    have = [t.cpu() for t in s.nbest(final_rows=range(B8))]
    for name, a, w, o in zip(NAMES, have, want, other):
        for b in range(B8):
            if b != 3:
                np.testing.assert_array_equal(bits(a[b]), bits(w[b]), err_msg=f"{name} stream {b}")
        if name == "tokens":
            assert torch.equal(a[3, :, :23], o[0]) and not a[3, :, 23:].any()
        else:
            np.testing.assert_array_equal(bits(a[3]), bits(o[0]), err_msg=name)


# ------------------------------------------------------------------------------------------------------------------ 3: zero weights
@pytest.mark.parametrize("V", [29, 1000])
def test_zero_weights_give_the_plain_stream(dev, V):
    rng = np.random.default_rng(50 + V)
    committed = 0
    for W in (1, 4, 32):
        for blank in (0, V - 1):
            tables = O.markov_lm(V, blank, 3, seed=3).tables(0.0, 0.0)
            x = torch.from_numpy((rng.standard_normal((B8, T60, V)) * 3.0).astype(np.float32)).to(dev)
            C = 7
            s = K.CtcLmBeamStream(B8, C, T60, V, W, tables, blank_index=blank, device=dev)
            p = K.CtcBeamStream(B8, C, T60, V, W, blank_index=blank, device=dev)
            steps = plan(LENS, C)
            for i, (start, nv) in enumerate(steps):
                xc = chunk_of(x, start, nv, C)
                s.advance(xc, nv)
                p.advance(xc, nv)
                last = i == len(steps) - 1
                fin = range(B8) if last else [b for b in range(B8) if s.frames[b] == LENS[b] and i % 2]
                tk, n, score, lp, ls = s.nbest(final_rows=fin)
                ptk, pn, plp = p.nbest()
                assert torch.equal(tk, ptk) and torch.equal(n, pn), (V, W, blank, i)
                np.testing.assert_array_equal(bits(lp), bits(plp))
                np.testing.assert_array_equal(bits(score), bits(plp))
                assert not ls.any()
                a, b_ = s.commit(final_rows=range(B8) if last else ()), p.commit(final_rows=range(B8) if last else ())
                assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]), (V, W, blank, i)
                committed += int(a[1].sum())
            assert torch.equal(s.committed, p.committed)
    assert committed > 0


# ------------------------------------------------------------------------------------------------------------------ 4: prefix re-entry while carried
def test_prefix_reentry_while_carried(dev):
    """the logits of test_ctc_lm_beam_gpu.test_prefix_reentry_small_alphabet_narrow_beam, cut into chunks of 1 and of 5: a prefix that
    leaves the beam and comes back in a later chunk finds its node, with its mass, its lm and its LM state"""
    rng = np.random.default_rng(5)
    tables = O.markov_lm(3, 0, 3, seed=2).tables(0.7, 0.2)
    B, T, V = 300, 14, 3
    for W in (2, 3):
        x = (rng.standard_normal((B, T, V)) * 1.5).astype(np.float32)
        h = O.host_lm(x, [T] * B, tables, W, 0, top_paths=W)
        xd = torch.from_numpy(x).to(dev)
        for C in (1, 5):
            s = K.CtcLmBeamStream(B, C, T, V, W, tables, blank_index=0, device=dev)
            for t0 in range(0, T, C):
                n = min(C, T - t0)
                s.advance(xd[:, t0:t0 + n].contiguous(), [n] * B)
            d = [t.cpu().numpy() for t in s.nbest(final_rows=range(B))]
            np.testing.assert_array_equal(d[1], h[1])
            np.testing.assert_array_equal(d[0], h[0])
            np.testing.assert_array_equal(d[4], h[4])
            np.testing.assert_allclose(d[3], h[3], rtol=0, atol=1e-4)
            np.testing.assert_array_equal(d[2], (d[3] + d[4]).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------------ 5: commit
def test_commits_follow_the_fused_best_row(dev):
    V, W, blank, C = 29, 4, 0, 7
    rng = np.random.default_rng(77)
    x = torch.from_numpy((rng.standard_normal((B8, T60, V)) * 2.0).astype(np.float32)).to(dev)
    tables = O.markov_lm(V, blank, 3, seed=3).tables(1.2, -0.6)
    want = [t.cpu() for t in one_shot(x, LENS, tables, W, blank)]
    plain = [t.cpu() for t in K.ctc_beam_search_device(x, LENS, W, W, blank)]
    fused_top = [tuple(want[0][b, 0, :int(want[1][b, 0])].tolist()) for b in range(B8)]
    # input conditions: a commit that ranks by the acoustic total would emit another row
    assert any(int(want[3][b].argmax()) != 0 for b in range(B8)), "in some final beam the acoustically best row is not the fused-best row"
    assert any(fused_top[b] != tuple(plain[0][b, 0, :int(plain[1][b, 0])].tolist()) for b in range(B8)), \
        "for some utterance the plain search's top path is not the fused search's"
    s = K.CtcLmBeamStream(B8, C, T60, V, W, tables, blank_index=blank, device=dev)
    got = [[] for _ in range(B8)]
    early = 0
    for start, nv in plan(LENS, C):
        s.advance(chunk_of(x, start, nv, C), nv)
        take(s, got)
        live = rows_of(*s.nbest()[:3])
        for b in range(B8):
            assert all(y[:len(got[b])] == tuple(got[b]) for y in live[b]), (b, got[b], live[b])
        early = sum(len(g) for g in got)
    take(s, got, final_rows=range(B8))
    assert [tuple(g) for g in got] == fused_top
    assert 0 < early < sum(len(g) for g in got)
    # the horizon commit's final flag ranks the same way
    s = K.CtcLmBeamStream(B8, C, T60, V, W, tables, blank_index=blank, device=dev)
    feed(s, x, LENS, C)
    got = [[] for _ in range(B8)]
    take(s, got, final_rows=range(B8), horizon=T60)
    assert [tuple(g) for g in got] == fused_top


# ------------------------------------------------------------------------------------------------------------------ 6: compaction
@pytest.mark.parametrize("final", [False, True])
def test_a_compaction_moves_the_lm_payload(dev, final):
    Tcap, H, T, W, C = 16, 8, 60, 4, 4
    x, lm = SO.rule_inputs()
    B, V, blank = len(x), SO.RULE_V, SO.RULE_BLANK
    tables = lm.tables(*SO.RULE_WEIGHTS)
    xd = torch.from_numpy(x).to(dev)
    s = K.CtcLmBeamStream(B, C, Tcap, V, W, tables, blank_index=blank, device=dev)
    got = [[] for _ in range(B)]
    fin = range(B) if final else None
    compactions = dropped = 0
    for t0 in range(0, T, C):
        over = [b for b in range(B) if s.frames[b] + C > Tcap]
        if over:
            before = [t.cpu() for t in s.nbest(final_rows=fin)]
            had = [len(d) for d in s.dropped]
            res = s.compact(over)
            after = [t.cpu() for t in s.nbest(final_rows=fin)]
            compactions += 1
            for b in range(B):
                drop, nodes, frames = res[b]
                assert nodes <= 1 + W * frames and frames == s.frames[b] <= Tcap
                assert len(s.dropped[b]) == had[b] + drop and (b in over or drop == 0)
                head = s.dropped[b][had[b]:]
                dropped += drop
                for p in range(W):
                    n0, n1 = int(before[1][b, p]), int(after[1][b, p])
                    live = float(before[3][b, p]) != -np.inf
                    assert n0 == n1 + (drop if live else 0), (t0, b, p)
                    assert before[0][b, p, :n0].tolist() == (head if live else []) + after[0][b, p, :n1].tolist(), (t0, b, p)
                    assert not after[0][b, p, n1:].any()
                for i in (2, 3, 4):  # score, log_prob, lm_score: the bits they had
                    np.testing.assert_array_equal(bits(after[i][b]), bits(before[i][b]), err_msg=f"t0={t0} stream {b} {NAMES[i]}")
        s.advance(xd[:, t0:t0 + C].contiguous(), [C] * B)
        take(s, got, horizon=H)
    assert compactions > 1 and dropped > 0
    assert all(got[b][:len(s.dropped[b])] == s.dropped[b] for b in range(B))  # what left the trie had been committed


# ------------------------------------------------------------------------------------------------------------------ 7: the horizon rule under fusion
@pytest.mark.parametrize("W,H,C,Tcap", SO.RULE_CASES)
def test_horizon_rule_under_fusion_against_the_oracle(dev, W, H, C, Tcap):
    """SO.RULE_SEEDS: smallest oracle margin >= 1e-3 over every case (pinned on the CPU by test_ctc_lm_stream_oracle.py); _against_oracle
    asserts >= 1e-4 for this case's runs, and that some prune point removes a row and some leaves the common ancestor in charge"""
    x, lm = SO.rule_inputs()
    B, T, V, blank = len(x), SO.RULE_T, SO.RULE_V, SO.RULE_BLANK
    runs = SO.rule_runs(W, H, C, Tcap)
    xd = torch.from_numpy(x).to(dev)
    s = K.CtcLmBeamStream(B, C, Tcap or T, V, W, lm.tables(*SO.RULE_WEIGHTS), blank_index=blank, device=dev)
    compactions = []

    def feed_chunk(i):
        n = min(C, T - i * C)
        over = [b for b in range(B) if s.frames[b] + n > (Tcap or T)]
        if over:
            s.compact(over)
            compactions.append(i)
        s.advance(xd[:, i * C:i * C + n].contiguous(), [n] * B)
        return [n] * B

    _against_oracle(s, feed_chunk, runs, W, H, (W, H, C, Tcap))
    assert sum(r["flips"] for r in runs) > 0, "input condition: at some prune point the fused-best row is not the acoustically best row"
    assert bool(compactions) == (Tcap is not None)
    rows, (score, lp, ls) = full_beam(s, W)  # after the last prune point: the running order, and its parts
    for b in range(B):
        live, parts = runs[b]["steps"][-1][2], runs[b]["parts"][-1]
        assert rows[b] == [y for y, _ in live]
        np.testing.assert_allclose(lp[b, :len(live)].numpy(), [a for a, _ in parts], rtol=1e-3, atol=1e-3)
        np.testing.assert_allclose(ls[b, :len(live)].numpy(), [l for _, l in parts], rtol=1e-3, atol=1e-3)
    tk, n, score, lp, ls = [t.cpu() for t in s.nbest(final_rows=range(B))]  # the streams have ended: the order with the term
    for b in range(B):
        final = runs[b]["final"]
        have = [tuple(s.dropped[b]) + tuple(tk[b, p, :int(n[b, p])].tolist()) for p in range(len(final))]
        assert have == [y for y, *_ in final], (b, have, final)
        for i, t in ((1, score), (2, lp), (3, ls)):
            np.testing.assert_allclose(t[b, :len(final)].numpy(), [r[i] for r in final], rtol=1e-3, atol=1e-3)
