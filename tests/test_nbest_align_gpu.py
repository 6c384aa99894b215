"""tfasr_row_lse_entropy / tfasr_ctc_nbest_align on the device (csrc/align.hip, csrc/ctc.hip).

1. Bit for bit against tfasr_ctc_align run once per path on the utterance's logits (start, end, label_lp, score), on every launch shape
   of the walk, with ragged frames, empty label rows, repeats that fit exactly or miss by a frame, and the labels read in place from a
   [B, P, T] token array (ldl = T > U).
2. Dead rows (label_len -1) and over-long rows give -inf / -1 / 0 and leave their neighbours alone.
3. Against the f64 oracle (tests/nbest_detail_oracle.py) exactly, on dyadic log-probabilities: logits that are multiples of 1/8 in
   [-8, 0] plus one class at +64 that no path visits.  Its exp dominates the frame's sum so completely that the f32 and the f64 lse
   are both exactly 64, every log-probability x - 64 is exact, and so is every sum of them: ties are real and the spans must match.
4. On random floats against the oracle, within TWICE the error the parent's kernels (tfasr_ctc_align for the sums and the score,
   tfasr_ctc_greedy_decode_detail for the mean entropies) show against the same oracle on the same logits: the new kernel performs the
   same additions.  Both numbers go to profiles/nbest_detail_parity.json.
5. tfasr_row_lse_entropy: the lse through single-frame alignments whose score is x[blank] - lse, bit for bit; the entropy against f64
   within twice the greedy detail decoder's error on the same rows (single-frame tokens carry the frame's entropy).
6. The greedy transcript as the only hypothesis: the spans of tfasr_ctc_greedy_decode_detail exactly, its sums and entropies within
   the bounds of 4."""
import numpy as np
import pytest
import torch

import nbest_detail_oracle as O
from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

pytestmark = pytest.mark.gpu
I32 = torch.int32
NEG = float("-inf")


def dv(dev, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def per_path(logits, logit_len, tokens, lengths, blank, U):
    """tfasr_ctc_align once per path on the utterance's logits -> start, end, label_lp [B, P, U], score [B, P]"""
    outs = [K.ctc_align(logits, tokens[:, p, :U].contiguous(), lengths[:, p].clamp(0, U).contiguous(), logit_len, blank=blank)
            for p in range(tokens.shape[1])]
    outs = [[x.clone() for x in o] for o in outs]
    return [torch.stack([o[i] for o in outs], 1) for i in range(4)]


def assert_same_as_per_path(logits, logit_len, tokens, lengths, blank, U):
    got = K.ctc_nbest_align(logits, logit_len, tokens, lengths, blank=blank, max_labels=U)
    got = [x.clone() for x in got]
    want = per_path(logits, logit_len, tokens, lengths, blank, U)
    for name, g, w in zip(("start", "end", "label_lp", "score"), (got[0], got[1], got[2], got[4]), want):
        assert g.shape == w.shape and torch.equal(g, w), name
    ent = got[3]
    assert (ent[got[0] < 0] == 0).all() and torch.isfinite(ent).all() and (ent >= 0).all()
    return got


def labels_without_repeats(rng, n, V, blank):
    cls = [c for c in range(V) if c != blank]
    out = [cls[rng.integers(len(cls))]]
    while len(out) < n:
        c = cls[rng.integers(len(cls))]
        if c != out[-1]:
            out.append(c)
    return out


# ------------------------------------------------------------------------------------------------------------------ 1. per path
@pytest.mark.parametrize("tl", [[40, 17, 33], [40, 1, 0]], ids=["ragged", "one_and_no_frames"])
@pytest.mark.parametrize("blank", [0, 6])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_base_shape_is_tfasr_ctc_align_per_path(dev, dtype, blank, tl):
    B, P, T, V, U = 3, 4, 40, 7, 21
    rng = np.random.default_rng([blank, tl[1]])
    logits = dv(dev, (rng.standard_normal((B, T, V)) * 2).astype(np.float32), dtype)
    cls = [c for c in range(V) if c != blank]
    tokens = rng.choice(cls, (B, P, T)).astype(np.int32)
    lengths = np.zeros((B, P), np.int32)
    for b in range(B):
        half = (tl[b] + 1) // 2
        lengths[b, 0] = rng.integers(1, 9)
        lengths[b, 1] = 0
        tokens[b, 2, :half] = cls[1]  # repeats, a blank between each pair: 2 * half - 1 frames (an odd frame count fits exactly)
        lengths[b, 2] = half
        tokens[b, 3, :half] = cls[2]  # one label more: a frame short when the row above fits exactly
        tokens[b, 3, half] = cls[3]
        lengths[b, 3] = half + 1
    got = assert_same_as_per_path(logits, dv(dev, np.asarray(tl, np.int32)), dv(dev, tokens), dv(dev, lengths), blank, U)
    score = got[4].cpu().numpy()
    for b in range(B):
        if tl[b] == 0:
            assert (score[b] == NEG).all() and (got[0][b] == -1).all()
        elif tl[b] % 2:
            assert np.isfinite(score[b, 2]) and score[b, 3] == NEG  # fits exactly / misses by a frame
            assert got[0][b, 2, :lengths[b, 2]].tolist() == list(range(0, tl[b], 2))
            assert (got[0][b, 3] == -1).all() and (got[1][b, 3] == -1).all() and (got[2][b, 3] == 0).all()
        else:
            assert np.isfinite(score[b, 2]) and np.isfinite(score[b, 3])
        if tl[b] > 0:
            assert np.isfinite(score[b, 1]) and (got[0][b, 1] == -1).all()  # no labels: the all-blank path


@pytest.mark.parametrize("U", [31, 32, 63, 64])
def test_thread_count_edges_of_the_walk(dev, U):
    B, P, T, V = 2, 3, 140, 5
    rng = np.random.default_rng(U)
    logits = dv(dev, (rng.standard_normal((B, T, V)) * 2).astype(np.float32))
    tokens = rng.integers(1, V, (B, P, T)).astype(np.int32)
    lengths = np.array([[U, U // 2, 0], [U - 1, U, 1]], np.int32)
    got = assert_same_as_per_path(logits, dv(dev, np.asarray([T, T - 9], np.int32)), dv(dev, tokens), dv(dev, lengths), 0, U)
    assert torch.isfinite(got[4]).all()  # 2U + 1 <= 129 frames: every row fits whatever its repeats


def test_widest_label_row(dev):
    B, P, T, V, U = 1, 2, 600, 5, 511
    rng = np.random.default_rng(511)
    logits = dv(dev, (rng.standard_normal((B, T, V)) * 2).astype(np.float32))
    tokens = np.zeros((B, P, T), np.int32)
    tokens[0, 0, :U] = labels_without_repeats(rng, U, V, 0)
    tokens[0, 1, :300] = rng.integers(1, V, 300)
    lengths = np.array([[U, 300]], np.int32)
    got = assert_same_as_per_path(logits, dv(dev, np.asarray([T], np.int32)), dv(dev, tokens), dv(dev, lengths), 0, U)
    assert torch.isfinite(got[4][0, 0])
    with pytest.raises(_lib.TfasrUnsupported):
        K.ctc_nbest_align(logits, dv(dev, np.asarray([T], np.int32)), dv(dev, tokens), dv(dev, lengths), max_labels=U + 1)


def test_default_width_fills_the_columns_past_the_limit(dev):
    B, P, T, V = 1, 2, 520, 4
    rng = np.random.default_rng(2)
    logits = dv(dev, rng.standard_normal((B, T, V)).astype(np.float32))
    tokens = dv(dev, rng.integers(1, V, (B, P, T)).astype(np.int32))
    lengths = dv(dev, np.array([[7, 515]], np.int32))
    start, end, lp, ent, score = K.ctc_nbest_align(logits, dv(dev, np.asarray([T], np.int32)), tokens, lengths)
    assert start.shape == (B, P, T) and ent.shape == (B, P, T)
    assert (start[:, :, 511:] == -1).all() and (end[:, :, 511:] == -1).all() and (lp[:, :, 511:] == 0).all() and (ent[:, :, 511:] == 0).all()
    assert torch.isfinite(score[0, 0]) and score[0, 1] == NEG and (start[0, 1] == -1).all()  # 515 labels: too long to align


# ------------------------------------------------------------------------------------------------------------------ 2. dead rows
def test_dead_and_overlong_rows_leave_their_neighbours_alone(dev):
    B, P, T, V, U = 3, 4, 40, 7, 12
    rng = np.random.default_rng(4)
    logits = dv(dev, (rng.standard_normal((B, T, V)) * 2).astype(np.float32))
    tokens = dv(dev, rng.integers(1, V, (B, P, T)).astype(np.int32))
    tl = dv(dev, np.asarray([40, 25, 31], np.int32))
    live = np.array([[3, 5, 2, 6], [4, 1, 7, 2], [5, 5, 3, 0]], np.int32)
    marked = live.copy()
    marked[0, 1], marked[1, 0], marked[1, 3], marked[2, 2] = -1, U + 1, -7, T
    ref = [x.clone() for x in K.ctc_nbest_align(logits, tl, tokens, dv(dev, live), max_labels=U)]
    got = K.ctc_nbest_align(logits, tl, tokens, dv(dev, marked), max_labels=U)
    gone = torch.from_numpy(marked != live).to(dev)
    for r, g in zip(ref, got):
        assert torch.equal(r[~gone], g[~gone])
    start, end, lp, ent, score = got
    assert (score[gone] == NEG).all() and (start[gone] == -1).all() and (end[gone] == -1).all() and (lp[gone] == 0).all() and (ent[gone] == 0).all()
    assert torch.isfinite(ref[4]).all()


# ------------------------------------------------------------------------------------------------------------------ 3. exact
def dyadic_logits(rng, shape, sink, levels=65):
    """multiples of 1/8 in [-8, 0] (levels < 65: fewer values, more ties); class `sink` at +64 makes every frame's lse exactly 64"""
    step = 64 // (levels - 1)
    x = (-(rng.integers(0, levels, shape) * step) / 8.0).astype(np.float32)
    x[..., sink] = 64.0
    return x


@pytest.mark.parametrize("levels", [65, 3])
@pytest.mark.parametrize("blank", [0, 6])
def test_exact_against_the_oracle_on_dyadic_log_probabilities(dev, blank, levels):
    B, P, T, V, U, sink = 3, 4, 40, 7, 12, 3
    rng = np.random.default_rng([blank, levels])
    x = dyadic_logits(rng, (B, T, V), sink, levels)
    lse, _ = O.frame_stats(x)
    assert (lse == 64.0).all()  # in f64 too: log1p(6 e^-64) is far below an ulp of 64
    cls = [c for c in range(V) if c not in (blank, sink)]
    tokens = rng.choice(cls, (B, P, T)).astype(np.int32)
    lengths = rng.integers(0, U + 1, (B, P)).astype(np.int32)
    lengths[0, 0], lengths[1, 1], lengths[2, 3] = U, 0, -1
    tl = [40, 23, 31]
    start, end, lp, ent, score = [t.cpu().numpy() for t in
                                  K.ctc_nbest_align(dv(dev, x), dv(dev, np.asarray(tl, np.int32)), dv(dev, tokens), dv(dev, lengths), blank=blank,
                                                    max_labels=U)]
    ws, we, wl, wh, wsc = O.nbest_align(x, tl, tokens, lengths, blank, U)
    np.testing.assert_array_equal(start, ws)
    np.testing.assert_array_equal(end, we)
    np.testing.assert_array_equal(lp.astype(np.float64), wl)
    np.testing.assert_array_equal(score.astype(np.float64), wsc)
    np.testing.assert_allclose(ent, wh, rtol=0, atol=1e-20)  # 6 e^-64 (64 + 8): both are ~1e-25
    assert np.isfinite(wsc).sum() >= 8 and (wsc[2, 3] == -np.inf)


# ------------------------------------------------------------------------------------------------------------------ 4. random floats
def smooth_logits(rng, B, T, V, blank):
    """random logits whose arg-max holds for runs of 1-9 frames, blanks between some runs: greedy tokens with spans like an aligned label's"""
    x = (rng.standard_normal((B, T, V)) * 1.5).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(1, 10))
            c = blank if rng.random() < 0.35 else int(rng.integers(0, V))
            x[b, t:t + n, c] += 4.0
            t += n
    return x


@pytest.fixture(scope="module")
def parity(dev):
    """One random case, every kernel and the oracle on it once: the greedy transcript and two edited copies of it as the hypotheses."""
    B, P, T, V, blank = 4, 3, 80, 29, 0
    rng = np.random.default_rng(17)
    x = smooth_logits(rng, B, T, V, blank)
    tl = [80, 57, 80, 33]
    logits, tl_d = dv(dev, x), dv(dev, np.asarray(tl, np.int32))
    g_tok, g_len, g_start, g_end, g_lp, g_ent, g_score = [t.clone() for t in K.ctc_greedy_decode_detail(logits, tl_d, blank=blank)]
    tokens = np.zeros((B, P, T), np.int32)
    lengths = np.zeros((B, P), np.int32)
    gt, gl = g_tok.cpu().numpy(), g_len.cpu().numpy()
    for b in range(B):
        n = int(gl[b])
        hyp = gt[b, :n].tolist()
        sub = list(hyp)
        for i in range(1, n, 4):
            sub[i] = 1 + (sub[i] + 6) % (V - 1)  # every fourth token replaced
        dele = [c for i, c in enumerate(hyp) if i % 5 != 2]  # every fifth token dropped
        for p, h in enumerate((hyp, sub, dele)):
            tokens[b, p, :len(h)], lengths[b, p] = h, len(h)
    U = int(lengths.max())
    tok_d, len_d = dv(dev, tokens), dv(dev, lengths)
    new = [t.clone() for t in K.ctc_nbest_align(logits, tl_d, tok_d, len_d, blank=blank, max_labels=U)]
    old = per_path(logits, tl_d, tok_d, len_d, blank, U)
    want = O.nbest_align(x, tl, tokens, lengths, blank, U)
    lse, ent = O.frame_stats(x)
    gs, ge = g_start.cpu().numpy(), g_end.cpu().numpy()
    g_ent_want = np.zeros((B, T))
    g_lp_want = np.zeros((B, T))
    for b in range(B):
        for i in range(int(gl[b])):
            g_ent_want[b, i] = ent[b, gs[b, i]:ge[b, i]].mean()
            g_lp_want[b, i] = (x[b, gs[b, i]:ge[b, i], gt[b, i]].astype(np.float64) - lse[b, gs[b, i]:ge[b, i]]).sum()
    err = lambda a, w: float(np.abs(np.asarray(a.cpu().numpy(), np.float64) - w).max())  # noqa: E731
    fig = {
        "shape": dict(B=B, P=P, T=T, V=V, U=U),
        "parent_label_lp": err(old[2], want[2]), "parent_score": err(old[3], want[4]),
        "parent_greedy_tok_logp": err(g_lp, g_lp_want), "parent_greedy_tok_entropy": err(g_ent, g_ent_want),
        "new_label_lp": err(new[2], want[2]), "new_score": err(new[4], want[4]), "new_label_entropy": err(new[3], want[3]),
    }
    fig["bound_label_lp"], fig["bound_score"] = 2 * fig["parent_label_lp"], 2 * fig["parent_score"]
    fig["bound_label_entropy"] = 2 * fig["parent_greedy_tok_entropy"]
    fig["bound_label_lp_vs_greedy"] = 2 * max(fig["parent_label_lp"], fig["parent_greedy_tok_logp"])
    print("nbest detail parity:", fig)
    O.write_parity("ctc_nbest_align", fig)
    return dict(fig=fig, new=new, old=old, want=want, greedy=(g_tok, g_len, g_start, g_end, g_lp, g_ent, g_score), lengths=lengths, U=U,
                logits=logits, logit_len=tl_d, blank=blank)


def test_random_floats_within_twice_the_parents_error(parity):
    fig, new, want = parity["fig"], parity["new"], parity["want"]
    np.testing.assert_array_equal(new[0].cpu().numpy(), want[0])  # no ties on random floats: the oracle's spans
    np.testing.assert_array_equal(new[1].cpu().numpy(), want[1])
    assert np.isfinite(want[4]).all() and int(parity["lengths"].sum()) > 60  # every hypothesis fits; a few dozen tokens are judged
    assert fig["parent_label_lp"] > 0 and fig["parent_greedy_tok_entropy"] > 0  # (a bound of 0 would ask for more than f32 holds)
    assert fig["new_label_lp"] <= fig["bound_label_lp"], fig
    assert fig["new_score"] <= fig["bound_score"], fig
    assert fig["new_label_entropy"] <= fig["bound_label_entropy"], fig


def test_greedy_transcript_as_the_only_hypothesis(dev, parity):
    """The greedy decoder's own token array [B, 1, T] as a one-path list (P = 1, every column a label column): the greedy path is the best
    path overall, so the best alignment of what it collapses to.  Its spans exactly; its sums and mean entropies within the bounds."""
    g_tok, g_len, g_start, g_end, g_lp, g_ent, g_score = parity["greedy"]
    fig = parity["fig"]
    B, T = g_tok.shape
    start, end, lp, ent, score = K.ctc_nbest_align(parity["logits"], parity["logit_len"], g_tok.view(B, 1, T), g_len.view(B, 1), blank=parity["blank"])
    assert start.shape == (B, 1, T) and torch.isfinite(score).all() and int(g_len.sum()) > 30
    assert torch.equal(start[:, 0], g_start) and torch.equal(end[:, 0], g_end)
    assert float((lp[:, 0] - g_lp).abs().max()) <= fig["bound_label_lp_vs_greedy"], fig
    assert float((ent[:, 0] - g_ent).abs().max()) <= fig["bound_label_entropy"], fig
    for got, shared in zip((start, end, lp, ent), parity["new"][:4]):  # the same rows as path 0 of the three-path list
        assert torch.equal(got[:, 0, :parity["U"]], shared[:, 0])


# ------------------------------------------------------------------------------------------------------------------ 5. frame statistics
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [2, 29, 1000, 1027])
def test_row_lse_entropy(dev, V, dtype):
    rows, blank = 37, 0
    rng = np.random.default_rng(V)
    x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    x[:, blank] = x.min(1) - 1.0  # never the arg-max: every single-frame utterance decodes to one token that carries the frame's entropy
    x[1, 1] = 200.0  # one dominant class: exp(x - 200) underflows for every other class, which then contributes 0
    if V > 2:
        x[2, V - 1] = -np.inf
    xd = dv(dev, x, dtype)
    lse, ent = K.row_lse_entropy(xd)
    one = torch.ones(rows, dtype=I32, device=dev)
    # a single frame and no labels: score = x[blank] - lse in f32, the subtraction tfasr_ctc_align performs with ITS lse
    score = K.ctc_align(xd.view(rows, 1, V), torch.zeros(rows, 1, dtype=I32, device=dev), torch.zeros(rows, dtype=I32, device=dev), one, blank=blank)[3]
    assert torch.equal(score, xd[:, blank].float() - lse)
    lse3, ent3 = K.row_lse_entropy(xd.view(rows, 1, V))
    assert lse3.shape == (rows, 1) and torch.equal(lse3.view(-1), lse) and torch.equal(ent3.view(-1), ent)
    want_lse, want_ent = O.frame_stats(xd.double().cpu().numpy())
    g = K.ctc_greedy_decode_detail(xd.view(rows, 1, V), one, blank=blank)
    assert (g[1] == 1).all()
    parent = float(np.abs(g[5][:, 0].double().cpu().numpy() - want_ent).max())
    mine = float(np.abs(ent.double().cpu().numpy() - want_ent).max())
    mine_lse = float(np.abs(lse.double().cpu().numpy() - want_lse).max())
    print(f"row_lse_entropy V={V} {dtype}: entropy error {mine:.3e} (greedy detail decoder {parent:.3e}), lse error {mine_lse:.3e}")
    O.write_parity(f"row_lse_entropy_V{V}_{'f32' if dtype == torch.float32 else 'bf16'}",
                   dict(parent_greedy_frame_entropy=parent, new_entropy=mine, bound_entropy=2 * parent, new_lse=mine_lse))
    assert mine <= 2 * parent
    assert float(ent[1]) == 0.0 and float(lse[1]) == 200.0  # the underflow rule
    # lse = m + logf(s): s is a sum of at most V / 64 + 6 <= 23 f32 additions (relative error 23 * 2^-24 of s, the same absolute error of
    # its logarithm, < 2^-18), then logf and the final addition round once each in units of |lse|
    assert mine_lse <= 2.0 ** -22 * float(np.abs(want_lse).max()) + 2.0 ** -18
