"""Forced alignment on the device (csrc/align.hip) against numpy oracles written here.

The walks are judged EXACTLY, with no tolerance, through rnnt_align_lattice and ctc_align(normalized=True) on dyadic
log-probabilities (multiples of 1/8 in [-8, 0]: a sum of a thousand of them has 3 fractional bits and stays far below 2^24, so it
is exact in f32 and in f64, and ties are real, frequent and reproducible).  The models' align() is judged end to end by the f64
score of the device's own path, which needs no exclusion of near-ties.

Tie rules.  CTC: the smallest move wins (stay, then s-1, then s-2) and the final blank wins at the end, i.e. of all best paths the one
whose state sequence, read from the last frame backwards, is largest.  Transducer: a label is emitted as late as possible, i.e. of
all best paths the one with every label at its latest frame (best paths that cross share a node, so that one exists): in the
back-trace from (Tl-1, Ul) the label move into (t, u) is taken when both moves give the same value.  (Going FORWARD that path
prefers the blank move wherever a best path continues that way; taking the blank move in the BACK-trace on a tie would instead put
every label of an all-equal lattice at frame 0.  The all-equal lattice below pins the rule: every label at frame Tl-1.)"""
import itertools
import math

import numpy as np
import pytest
import torch

from tensorflowasr_amd import _lib, configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.contextnet import ContextNetTransducer
from tensorflowasr_amd.ctc_model import ConformerCTC
from tensorflowasr_amd.schemas import AlignOutput, PredictInput, TrainData, TrainInput, TrainLabel, token_times

pytestmark = pytest.mark.gpu
NEG = -np.inf
I32 = torch.int32


# ------------------------------------------------------------------------------------------------------------------ oracles
def rnnt_oracle(bl, tr, Tl, Ul, U):
    """Viterbi over blank / truth [T, >=Ul+1] (f64), anti-diagonal by anti-diagonal -> (frames [U], label_lp [U], score)."""
    frames, llp = np.full(U, -1, np.int32), np.zeros(U, np.float64)
    if Tl <= 0:
        return frames, llp, NEG
    v = np.full((Tl, Ul + 1), NEG)
    lab = np.zeros((Tl, Ul + 1), bool)
    v[0, 0] = 0.0
    for n in range(1, Tl + Ul):
        u = np.arange(max(0, n - Tl + 1), min(n, Ul) + 1)
        t = n - u
        tp, up = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
        xb = np.where(t > 0, v[tp, u] + bl[tp, u], NEG)
        xt = np.where(u > 0, v[t, up] + tr[t, up], NEG)
        lm = (u > 0) & ((t == 0) | (xt >= xb))  # a tie: the label at this (later) frame
        v[t, u] = np.where(lm, xt, xb)
        lab[t, u] = lm
    t, u = Tl - 1, Ul
    while u > 0:
        if lab[t, u]:
            frames[u - 1], llp[u - 1] = t, tr[t, u - 1]
            u -= 1
        else:
            t -= 1
    return frames, llp, v[Tl - 1, Ul] + bl[Tl - 1, Ul]


def rnnt_path_score(bl, tr, Tl, Ul, frames):
    """log-probability (and its terms) of the path that emits label u at frames[u]"""
    terms, u = [], 0
    for t in range(Tl):
        while u < Ul and frames[u] == t:
            terms.append(tr[t, u])
            u += 1
        terms.append(bl[t, u])
    assert u == Ul
    return float(np.sum(terms)), terms


def ctc_ext(labels, Ul, blank, V):
    lab = np.clip(np.asarray(labels[:Ul], np.int64), 0, V - 1)
    ext = np.full(2 * Ul + 1, blank, np.int64)
    ext[1::2] = lab
    skip = np.zeros(2 * Ul + 1, bool)
    skip[3::2] = lab[1:] != lab[:-1]
    return ext, skip


def ctc_oracle(lp, labels, Tl, Ul, U, blank):
    """Viterbi over log-probabilities lp [T, V] (f64) -> (start [U], end [U], label_lp [U], score, number of paths)."""
    start, end, llp = np.full(U, -1, np.int32), np.full(U, -1, np.int32), np.zeros(U, np.float64)
    if Tl <= 0:
        return start, end, llp, NEG, 0
    ext, skip = ctc_ext(labels, Ul, blank, lp.shape[1])
    S = len(ext)
    v = np.full(S, NEG)
    v[:2] = lp[0, ext[:2]]
    cnt = [0] * S  # python integers: the number of paths grows past 2^63
    for s in range(min(S, 2)):
        cnt[s] = 1
    mv = np.zeros((Tl, S), np.int8)
    for t in range(1, Tl):
        a1 = np.concatenate([[NEG], v[:-1]])
        a2 = np.where(skip, np.concatenate([[NEG, NEG], v[:-2]])[:S], NEG)
        best, m = v.copy(), np.zeros(S, np.int8)
        sel = a1 > best
        best[sel], m[sel] = a1[sel], 1
        sel = a2 > best
        best[sel], m[sel] = a2[sel], 2
        v, mv[t] = best + lp[t, ext], m
        cnt = [cnt[s] + (cnt[s - 1] if s >= 1 else 0) + (cnt[s - 2] if skip[s] else 0) for s in range(S)]
    a1, a2 = v[S - 1], (v[S - 2] if S >= 2 else NEG)
    score = max(a1, a2)
    npaths = cnt[S - 1] + (cnt[S - 2] if S >= 2 else 0)
    if score == NEG:
        return start, end, llp, NEG, npaths
    s = S - 2 if a2 > a1 else S - 1
    for t in range(Tl - 1, -1, -1):
        if s & 1:
            u = s >> 1
            if end[u] < 0:
                end[u] = t + 1
            start[u] = t
        s -= int(mv[t, s])
    for u in range(Ul):
        for t in range(start[u], end[u]):
            llp[u] = lp[t, ext[2 * u + 1]] if t == start[u] else llp[u] + lp[t, ext[2 * u + 1]]
    return start, end, llp, score, npaths


def ctc_path_score(lp, labels, Tl, Ul, blank, start, end):
    ext, _ = ctc_ext(labels, Ul, blank, lp.shape[1])
    state = np.full(Tl, blank, np.int64)
    for u in range(Ul):
        state[start[u]:end[u]] = ext[2 * u + 1]
    terms = lp[np.arange(Tl), state]
    return float(terms.sum()), terms


# ------------------------------------------------------------------------------------------------------------------ helpers
def dyadic(rng, shape, levels=65):
    """multiples of 1/8 in [-8, 0]; levels < 65 draws from fewer values (more ties)"""
    step = 64 // (levels - 1)
    return (-(rng.integers(0, levels, shape) * step) / 8.0).astype(np.float32)


def dv(dev, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def pack(dense, tl, ul):
    """dense [B,T,U1] -> the valid nodes of every utterance, row-major (t,u) with Ul+1 columns, and cell_off [B+1]"""
    B, T, U1 = dense.shape
    tl, ul = np.clip(tl, 0, T), np.clip(ul, 0, U1 - 1)
    flat = [dense[b, :tl[b], :ul[b] + 1].reshape(-1) for b in range(B)]
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum([len(f) for f in flat])
    return np.concatenate(flat).astype(np.float32), off


def run_rnnt_lattice(dev, bl, tr, tl, ul, packed):
    B, T, U1 = bl.shape
    tl_d, ul_d = dv(dev, np.asarray(tl, np.int32)), dv(dev, np.asarray(ul, np.int32))
    if packed:
        fb, off = pack(bl, tl, ul)
        ft, _ = pack(tr, tl, ul)
        out = K.rnnt_align_lattice(dv(dev, fb), dv(dev, ft), ul_d, tl_d, T=T, U1=U1, cell_off=dv(dev, off))
    else:
        out = K.rnnt_align_lattice(dv(dev, bl), dv(dev, tr), ul_d, tl_d)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def check_rnnt_exact(dev, bl, tr, tl, ul, packed):
    B, T, U1 = bl.shape
    frames, llp, score = run_rnnt_lattice(dev, bl, tr, tl, ul, packed)
    for b in range(B):
        Tl, Ul = min(max(tl[b], 0), T), min(max(ul[b], 0), U1 - 1)
        wf, wl, ws = rnnt_oracle(bl[b].astype(np.float64), tr[b].astype(np.float64), Tl, Ul, U1 - 1)
        np.testing.assert_array_equal(frames[b], wf, err_msg=f"frames of utterance {b} (Tl {Tl}, Ul {Ul})")
        np.testing.assert_array_equal(llp[b].astype(np.float64), wl, err_msg=f"label_lp of utterance {b}")
        assert float(score[b]) == ws, (b, Tl, Ul, score[b], ws)
        assert (np.diff(frames[b][:Ul]) >= 0).all()


def run_ctc(dev, lp, labels, tl, ul, blank=0, normalized=True):
    out = K.ctc_align(dv(dev, lp), dv(dev, np.asarray(labels, np.int32)), dv(dev, np.asarray(ul, np.int32)), dv(dev, np.asarray(tl, np.int32)),
                      blank=blank, normalized=normalized)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def check_ctc_exact(dev, lp, labels, tl, ul, blank=0):
    B, T, V = lp.shape
    U = labels.shape[1]
    start, end, llp, score = run_ctc(dev, lp, labels, tl, ul, blank)
    nofit = 0
    for b in range(B):
        Tl, Ul = min(max(tl[b], 0), T), min(max(ul[b], 0), U)
        ws_, we, wl, wsc, _ = ctc_oracle(lp[b].astype(np.float64), labels[b], Tl, Ul, U, blank)
        np.testing.assert_array_equal(start[b], ws_, err_msg=f"start of utterance {b} (Tl {Tl}, Ul {Ul})")
        np.testing.assert_array_equal(end[b], we, err_msg=f"end of utterance {b}")
        np.testing.assert_array_equal(llp[b].astype(np.float64), wl, err_msg=f"label_lp of utterance {b}")
        assert float(score[b]) == wsc, (b, Tl, Ul, score[b], wsc)
        nofit += wsc == NEG
    return nofit


# ------------------------------------------------------------------------------------------------------------------ 3. exact, random
def _ragged(rng, B, T, U):
    tl = rng.integers(1, T + 1, B)
    ul = rng.integers(0, U + 1, B)
    tl[0], ul[0] = T, U
    return tl.tolist(), ul.tolist()


RNNT_CASES = {
    # name: (B, T, U1, tl, ul)   None: drawn
    "ragged": (7, 12, 7, [12, 1, 0, 7, 12, 5, 1], [6, 3, 2, 0, 6, 6, 0]),
    "lengths_beyond_padding": (3, 6, 4, [9, 6, -2], [7, 3, 2]),
    "wave1_limit": (3, 9, 64, [9, 4, 1], [63, 40, 63]),
    "wave2_first": (3, 9, 65, [9, 4, 1], [64, 33, 64]),
    "wave2_limit": (3, 9, 128, [9, 4, 2], [127, 64, 100]),
    "wave4_first": (3, 9, 129, [9, 4, 2], [128, 65, 1]),
    "wave4_limit": (3, 40, 256, [40, 4, 17], [255, 128, 200]),
    "workgroup_first": (3, 40, 257, [40, 4, 17], [256, 129, 255]),
    "workgroup_limit": (2, 5, 1024, [5, 3], [1023, 700]),
    "bench": (32, 250, 65, None, None),
    "bench_long": (32, 743, 200, None, None),
}


@pytest.mark.parametrize("levels", [65, 3])
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("case", list(RNNT_CASES))
def test_rnnt_walk_is_exact_on_dyadic_lattices(dev, case, packed, levels):
    B, T, U1, tl, ul = RNNT_CASES[case]
    rng = np.random.default_rng([len(case), B, T, U1, levels])
    if tl is None:
        tl, ul = _ragged(rng, B, T, U1 - 1)
    bl, tr = dyadic(rng, (B, T, U1), levels), dyadic(rng, (B, T, U1), levels)
    check_rnnt_exact(dev, bl, tr, tl, ul, packed)


def test_rnnt_width_past_the_last_variant_is_unsupported(dev):
    z = torch.zeros(1, 2, 1025, device=dev)
    one = torch.ones(1, dtype=I32, device=dev)
    with pytest.raises(_lib.TfasrError):
        K.rnnt_align_lattice(z, z, one, one)


CTC_CASES = {
    # name: (B, T, U, V, tl, ul)
    "ragged": (7, 12, 5, 6, [12, 1, 0, 7, 12, 3, 1], [5, 1, 0, 0, 4, 5, 0]),
    "repeats": (6, 9, 4, 3, [9, 7, 6, 9, 4, 5], [4, 4, 4, 2, 4, 3]),  # labels in {1, 2}: repeats need a blank between them
    "lengths_beyond_padding": (3, 6, 3, 5, [9, 6, -2], [7, 3, 2]),
    "one_wave_limit": (3, 80, 31, 8, [80, 40, 62], [31, 20, 31]),
    "two_waves_first": (3, 80, 32, 8, [80, 40, 64], [32, 20, 32]),
    "widest": (2, 700, 511, 16, [700, 600], [511, 300]),
    "bench": (32, 250, 64, 1000, None, None),
    "bench_long": (8, 743, 199, 32, None, None),
}


@pytest.mark.parametrize("levels", [65, 3])
@pytest.mark.parametrize("case", list(CTC_CASES))
def test_ctc_walk_is_exact_on_dyadic_log_probabilities(dev, case, levels):
    B, T, U, V, tl, ul = CTC_CASES[case]
    rng = np.random.default_rng([len(case), B, T, U, V, levels])
    if tl is None:
        tl, ul = _ragged(rng, B, T, U)
    lp = dyadic(rng, (B, T, V), levels)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    nofit = check_ctc_exact(dev, lp, labels, tl, ul)
    if case == "repeats":
        assert nofit >= 1  # [1,1,..] in too few frames: score -inf, -1 everywhere


def test_ctc_repeated_labels_fit_exactly_or_not_at_all(dev):
    lp = dyadic(np.random.default_rng(3), (2, 5, 3))
    labels = np.array([[1, 1, 1], [1, 1, 1]], np.int32)
    start, end, llp, score = run_ctc(dev, lp, labels, [5, 4], [3, 3])
    np.testing.assert_array_equal(start, [[0, 2, 4], [-1, -1, -1]])  # label, blank, label, blank, label is the only path in 5 frames
    np.testing.assert_array_equal(end, [[1, 3, 5], [-1, -1, -1]])
    assert score[0] == lp[0, [0, 1, 2, 3, 4], [1, 0, 1, 0, 1]].astype(np.float64).sum() and score[1] == NEG
    np.testing.assert_array_equal(llp, [lp[0, [0, 2, 4], 1], [0, 0, 0]])
    check_ctc_exact(dev, lp, labels, [5, 4], [3, 3])


def test_ctc_other_blank_index_and_out_of_range_labels(dev):
    rng = np.random.default_rng(11)
    lp = dyadic(rng, (4, 10, 6), 3)
    labels = np.array([[1, 9, 2], [-4, 0, 3], [5, 5, 1], [2, 3, 4]], np.int32)  # clamped into [0, V) as the loss clamps them
    check_ctc_exact(dev, lp, labels, [10, 10, 8, 3], [3, 3, 3, 3], blank=5)


def test_ctc_width_past_the_limit_is_unsupported(dev):
    one = torch.ones(1, dtype=I32, device=dev)
    with pytest.raises(_lib.TfasrError):
        K.ctc_align(torch.zeros(1, 2, 4, device=dev), torch.ones(1, 512, dtype=I32, device=dev), one, one)


# ------------------------------------------------------------------------------------------------------------------ 4. pinned ties
def test_all_equal_transducer_lattice_puts_every_label_at_the_last_frame(dev):
    B, T, U1 = 4, 8, 5
    tl, ul = [8, 5, 1, 3], [4, 2, 4, 0]
    for packed in (False, True):
        x = np.full((B, T, U1), -1.0, np.float32)
        frames, llp, score = run_rnnt_lattice(dev, x, x, tl, ul, packed)
        for b in range(B):
            want = np.full(U1 - 1, -1, np.int32)
            want[:ul[b]] = tl[b] - 1
            np.testing.assert_array_equal(frames[b], want)
            np.testing.assert_array_equal(llp[b], np.where(want >= 0, -1.0, 0.0))
            assert score[b] == -(tl[b] + ul[b])


def test_ctc_tie_rule_by_hand(dev):
    """All log-probabilities 0, so every path ties.  Labels (1, 2), 4 frames, states b 1 b 2 b: the final blank wins the end; going back
    it stays until frame 2, where it was entered from state 3 (s-1); state 3 was entered at frame 1 by the only finite move, the skip
    from state 1 (stay and s-1 come from states not yet reachable).  Path: 1 2 b b.
    Labels (1, 1), 3 frames: no skip between equal labels, state 4 is out of reach, the path ends in state 3: 1 b 1."""
    lp = np.zeros((2, 4, 3), np.float32)
    labels = np.array([[1, 2], [1, 1]], np.int32)
    start, end, llp, score = run_ctc(dev, lp, labels, [4, 3], [2, 2])
    np.testing.assert_array_equal(start, [[0, 1], [0, 2]])
    np.testing.assert_array_equal(end, [[1, 2], [1, 3]])
    np.testing.assert_array_equal(score, [0.0, 0.0])
    np.testing.assert_array_equal(llp, np.zeros((2, 2)))
    # Label 2 at frame 1 now costs 1, so it moves to frame 2.  State 3 at frame 2 can be entered from the blank state 2 (s-1) or by the
    # skip from state 1 (s-2), both 0: the smaller move wins, and the blank state 2 was entered from state 1 at frame 1.  Path: 1 b 2 b.
    lp[0, 1, 2] = -1.0
    start, end, llp, score = run_ctc(dev, lp, labels, [4, 3], [2, 2])
    np.testing.assert_array_equal(start[0], [0, 2])
    np.testing.assert_array_equal(end[0], [1, 3])
    assert score[0] == 0.0


# ------------------------------------------------------------------------------------------------------------------ 5. brute force
def test_rnnt_brute_force_over_every_alignment(dev):
    shapes = [(Tl, Ul) for Tl in range(1, 7) for Ul in range(0, 5)]
    B, T, U1 = len(shapes), 6, 5
    for levels, seed in ((65, 0), (3, 1), (2, 2)):
        rng = np.random.default_rng(seed)
        bl, tr = dyadic(rng, (B, T, U1), levels), dyadic(rng, (B, T, U1), levels)
        tl, ul = [s[0] for s in shapes], [s[1] for s in shapes]
        frames, llp, score = run_rnnt_lattice(dev, bl, tr, tl, ul, packed=False)
        ties = 0
        for b, (Tl, Ul) in enumerate(shapes):
            paths = list(itertools.combinations_with_replacement(range(Tl), Ul))
            assert len(paths) == math.comb(Tl - 1 + Ul, Ul) <= 126
            totals = [rnnt_path_score(bl[b].astype(np.float64), tr[b].astype(np.float64), Tl, Ul, f)[0] for f in paths]
            best = max(totals)
            assert float(score[b]) == best, (Tl, Ul)
            winners = [f for f, s in zip(paths, totals) if s == best]
            ties += len(winners) > 1
            latest = tuple(np.max(np.array(winners).reshape(len(winners), Ul), axis=0)) if Ul else ()
            assert latest in winners  # best paths that cross share a node: every label at its latest frame is a best path
            assert tuple(frames[b][:Ul]) == latest, (Tl, Ul, winners)
        assert levels == 65 or ties >= 5  # the coarse draws do tie


def ctc_paths(ext, skip, Tl):
    S = len(ext)
    paths = [[s] for s in range(min(S, 2))]
    for _ in range(1, Tl):
        paths = [p + [s] for p in paths for s in (p[-1], p[-1] + 1, p[-1] + 2)
                 if s < S and (s - p[-1] < 2 or skip[s])]
    return [p for p in paths if p[-1] >= S - 2]


def test_ctc_brute_force_over_every_alignment(dev):
    shapes = [(Tl, Ul) for Tl in range(1, 7) for Ul in range(0, 5)]
    B, T, U, V = len(shapes), 6, 4, 3
    for levels, seed in ((65, 0), (3, 1), (2, 2)):
        rng = np.random.default_rng(seed)
        lp = dyadic(rng, (B, T, V), levels)
        labels = rng.integers(1, V, (B, U)).astype(np.int32)
        tl, ul = [s[0] for s in shapes], [s[1] for s in shapes]
        start, end, llp, score = run_ctc(dev, lp, labels, tl, ul)
        for b, (Tl, Ul) in enumerate(shapes):
            ext, skip = ctc_ext(labels[b], Ul, 0, V)
            paths = ctc_paths(ext, skip, Tl)
            _, _, _, _, npaths = ctc_oracle(lp[b].astype(np.float64), labels[b], Tl, Ul, U, 0)
            assert npaths == len(paths)  # (the oracle's path count, used against the loss below)
            if not paths:
                assert score[b] == NEG and (start[b] == -1).all() and (end[b] == -1).all()
                continue
            x = lp[b].astype(np.float64)
            totals = [x[np.arange(Tl), ext[p]].sum() for p in paths]
            best = max(totals)
            assert float(score[b]) == best, (Tl, Ul)
            # smallest move first, seen from the end: the largest state sequence read backwards
            choice = max((p for p, s in zip(paths, totals) if s == best), key=lambda p: p[::-1])
            for u in range(Ul):
                on = [t for t in range(Tl) if choice[t] == 2 * u + 1]
                assert (start[b, u], end[b, u]) == (on[0], on[-1] + 1), (Tl, Ul, choice)
                assert float(llp[b, u]) == x[on, ext[2 * u + 1]].sum()


# ------------------------------------------------------------------------------------------------------------------ models
def tiny(kind, dev, dtype=torch.float32, seed=0, gain=3.0, **over):
    """tiny model with a peaky joint and a token-sensitive prediction network, as the beam-search tests build it"""
    if kind == "conformer":
        model = ConformerTransducer(configs.conformer_tiny(**over), dev, dtype=dtype, seed=seed)
    else:
        model = ContextNetTransducer(configs.contextnet_tiny(**over), dev, dtype=dtype, seed=seed)
    with torch.no_grad():
        model.ps.p("joint/vocab/w").mul_(gain)
        model.ps.p("pred/emb").mul_(gain)
    model.ps.refresh_shadow()
    return model


def batch(V, lens, ulens, U, seed):
    rng = np.random.default_rng(seed)
    B = len(lens)
    sig = np.clip(rng.standard_normal((B, max(lens))) * 0.1, -1, 1).astype(np.float32)
    labels = rng.integers(1, V, (B, U)).astype(np.int32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0.0
        labels[b, ulens[b]:] = 0
    preds = np.concatenate([np.zeros((B, 1), np.int32), labels], 1)
    return TrainData(TrainInput(torch.from_numpy(sig), torch.tensor(lens, dtype=I32), torch.from_numpy(preds),
                                torch.tensor([u + 1 for u in ulens], dtype=I32)),
                     TrainLabel(torch.from_numpy(labels), torch.tensor(ulens, dtype=I32))), labels


def f64_lattice(model, data, labels):
    """blank / truth log-probabilities [B,T,U1] in f64 from the model's own logits, and its frame counts"""
    out = model(data.inputs)
    x = out.logits.double().cpu().numpy()
    lp = x - (x.max(-1, keepdims=True) + np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)))
    B, T, U1, V = x.shape
    tr = np.full((B, T, U1), NEG)
    for b in range(B):
        for u in range(U1 - 1):
            tr[b, :, u] = lp[b, :, u, labels[b, u]]
    return lp[..., 0], tr, [min(int(v), T) for v in out.logits_length.tolist()], x


def check_transducer_alignment(model, data, labels, ulens, out, route):
    """6: valid paths, and the f64 score of the device's own path within tol of the f64 optimum and of the reported score"""
    assert isinstance(out, AlignOutput) and out.ends is None
    bl, tr, tl, x = f64_lattice(model, data, labels)
    frames, llp, score = out.frames.cpu().numpy(), out.label_log_probs.cpu().numpy(), out.scores.cpu().numpy()
    U = frames.shape[1]
    assert out.seconds_per_frame == pytest.approx(model.cfg.time_reduction_factor * model.cfg.stride_ms / 1000.0)
    figures = []
    for b, Ul in enumerate(ulens):
        Tl = tl[b]
        f = frames[b]
        assert (f[Ul:] == -1).all() and (f[:Ul] >= 0).all() and (f[:Ul] < Tl).all() and (np.diff(f[:Ul]) >= 0).all(), (b, f, Tl)
        mine, terms = rnnt_path_score(bl[b], tr[b], Tl, Ul, f)
        _, _, opt = rnnt_oracle(bl[b], tr[b], Tl, Ul, U)
        n = Tl + Ul + 1
        if route == "f32":  # n f32 additions of the path's terms, doubled for the f32 log-softmax behind every term
            tol = 2 * n * 2.0 ** -23 * float(np.abs(terms).sum())
        else:  # every logit carries one bf16 rounding (the statistics come from the f32 accumulators, the oracle's logits are bf16)
            tol = n * 2.0 ** -8 * float(np.abs(x[b, :Tl, :Ul + 1]).max())
        figures.append((b, Tl, Ul, opt - mine, abs(float(score[b]) - mine), tol))
        print(f"align[{route}] b={b} Tl={Tl} Ul={Ul}: optimum - path {opt - mine:.3e}, |score - path| {abs(float(score[b]) - mine):.3e}, tol {tol:.3e}")
        assert mine <= opt + 1e-12
        assert opt - mine <= tol, figures[-1]
        assert abs(float(score[b]) - mine) <= tol, figures[-1]
        np.testing.assert_allclose(llp[b, :Ul], [tr[b, f[u], u] for u in range(Ul)], atol=tol, rtol=0)
        assert (llp[b, Ul:] == 0).all()
    t = token_times(out).cpu().numpy()
    np.testing.assert_allclose(t, np.where(frames >= 0, frames * out.seconds_per_frame, -1.0), rtol=1e-6)
    return figures


LENS, ULENS, UMAX = [4000, 4000, 2500, 3200], [4, 2, 3, 0], 4


@pytest.mark.parametrize("kind", ["conformer", "contextnet"])
def test_transducer_align_f32_end_to_end(dev, kind):
    model = tiny(kind, dev, torch.float32, seed=1)
    data, labels = batch(model.cfg.vocab_size, LENS, ULENS, UMAX, seed=4)
    check_transducer_alignment(model, data, labels, ULENS, model.align(data), "f32")


def test_batch_without_any_label_scores_the_all_blank_path(dev):
    model = tiny("conformer", dev, torch.float32, seed=1)
    data, labels = batch(model.cfg.vocab_size, LENS[:2], [0, 0], 1, seed=4)
    empty = TrainData(TrainInput(data.inputs.inputs, data.inputs.inputs_length, data.inputs.predictions[:, :1], data.inputs.predictions_length),
                      TrainLabel(data.labels.labels[:, :0], data.labels.labels_length))
    out = model.align(empty)
    assert out.frames.shape == (2, 0) and out.label_log_probs.shape == (2, 0)
    bl, tr, tl, x = f64_lattice(model, empty, labels[:, :0])
    for b in range(2):
        want = bl[b, :tl[b], 0].sum()
        assert abs(float(out.scores[b]) - want) <= 2 * (tl[b] + 1) * 2.0 ** -23 * np.abs(bl[b, :tl[b], 0]).sum()


@pytest.mark.parametrize("kind", ["conformer", "contextnet"])
def test_bf16_model_aligns_on_its_f32_twin_by_default(dev, kind):
    model = tiny(kind, dev, torch.bfloat16, seed=1)
    data, labels = batch(model.cfg.vocab_size, LENS, ULENS, UMAX, seed=4)
    check_transducer_alignment(model.inference_twin(), data, labels, ULENS, model.align(data), "f32")


def _count_calls(monkeypatch, name):
    calls = []
    real = getattr(K, name)

    def wrapped(*a, **k):
        calls.append(name)
        return real(*a, **k)

    monkeypatch.setattr(K, name, wrapped)
    return calls


@pytest.mark.parametrize("kind", ["conformer", "contextnet"])
def test_transducer_align_bf16_statistics_route_end_to_end(dev, kind, monkeypatch):
    # V % 8 == 0: the vocabulary product has its statistics epilogue (at these few rows the 128-row kernel, which also stores the logits)
    model = tiny(kind, dev, torch.bfloat16, seed=1, vocab_size=32)
    data, labels = batch(32, LENS, ULENS, UMAX, seed=4)
    stats_calls, plain_calls = _count_calls(monkeypatch, "rnnt_align_stats"), _count_calls(monkeypatch, "rnnt_align")
    out = model.align(data, precision="bf16")
    assert stats_calls and not plain_calls  # the walk never read logits
    check_transducer_alignment(model, data, labels, ULENS, out, "bf16")


def test_bf16_falls_back_to_materialised_logits_where_the_epilogue_does_not_apply(dev, monkeypatch):
    model = tiny("conformer", dev, torch.bfloat16, seed=1)  # V = 29
    data, labels = batch(model.cfg.vocab_size, LENS, ULENS, UMAX, seed=4)
    plain_calls = _count_calls(monkeypatch, "rnnt_align")
    out = model.align(data, precision="bf16")
    assert plain_calls
    check_transducer_alignment(model, data, labels, ULENS, out, "bf16")


def test_statistics_route_agrees_with_materialised_route(dev, monkeypatch):
    """7: equal frames for every utterance whose f64 gap between the best and the second-best path exceeds the bf16 bound of 6; at
    most 1 utterance in 8 may fall under that gap.  Model seed, gain and batch are fixed; the f64 oracle alone puts 2 of these 16
    utterances under their bound (gaps 0.53 and 0.19 against bounds 0.53 and 0.78; the closest one above is 0.82 against 0.70)."""
    lens = [3553, 2876, 4053, 5512, 3575, 5247, 3628, 5031, 3134, 3935, 3445, 3143, 5256, 4966, 2846, 5355]
    ulens = [3, 1, 2, 2, 2, 2, 1, 3, 3, 1, 3, 3, 1, 2, 2, 1]
    model = tiny("conformer", dev, torch.bfloat16, seed=1, gain=10.0, vocab_size=192, joint_dim=128)
    data, labels = batch(192, lens, ulens, 3, seed=21)
    stats_calls = _count_calls(monkeypatch, "rnnt_align_stats")
    a = model.align(data, precision="bf16")
    assert stats_calls
    model.fuse_joint_stats = False
    plain_calls = _count_calls(monkeypatch, "rnnt_align")
    b = model.align(data, precision="bf16")
    model.fuse_joint_stats = True
    assert plain_calls and len(stats_calls) == 1
    bl, tr, tl, x = f64_lattice(model, data, labels)
    fa, fb = a.frames.cpu().numpy(), b.frames.cpu().numpy()
    under = 0
    for i, Ul in enumerate(ulens):
        Tl = tl[i]
        totals = sorted((rnnt_path_score(bl[i], tr[i], Tl, Ul, f)[0] for f in itertools.combinations_with_replacement(range(Tl), Ul)), reverse=True)
        gap = totals[0] - totals[1] if len(totals) > 1 else np.inf
        tol = (Tl + Ul + 1) * 2.0 ** -8 * float(np.abs(x[i, :Tl, :Ul + 1]).max())
        print(f"routes b={i} Tl={Tl} Ul={Ul}: gap {gap:.3e}, bound {tol:.3e}, equal {np.array_equal(fa[i], fb[i])}")
        if gap > tol:
            np.testing.assert_array_equal(fa[i], fb[i])
        else:
            under += 1
    assert under * 8 <= len(ulens), under
    np.testing.assert_allclose(a.scores.cpu().numpy(), b.scores.cpu().numpy(), atol=max(
        (tl[i] + ulens[i] + 1) * 2.0 ** -8 * float(np.abs(x[i]).max()) for i in range(len(ulens))), rtol=0)


def test_statistics_only_route_at_the_bench_width(dev):
    """The vocabulary product with out=None (its 256-row kernel: the logits never exist) feeding rnnt_align_stats, on a packed ragged
    lattice at V = 1000, J = 320: judged as in 6 by the f64 score of the device's own path, on the f64 log-softmax of the SAME
    product materialised in bf16, so every logit differs by one bf16 rounding: tol = n * 2^-8 * max|logit|."""
    g = torch.Generator().manual_seed(5)
    B, T, U1, V, J = 32, 250, 33, 1000, 320  # (the 256-row kernel takes products of at least two tiles per CU)
    rng = np.random.default_rng(8)
    tl, ul = _ragged(rng, B, T, U1 - 1)
    off = np.zeros(B + 1, np.int64)
    off[1:] = np.cumsum([t * (u + 1) for t, u in zip(tl, ul)])
    total = int(off[-1])
    h = (torch.randn(total, J, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    W = (torch.randn(J, V, generator=g) * 0.3).to(dev).to(torch.bfloat16)
    bias = torch.randn(V, generator=g).to(dev)
    labels = rng.integers(1, V, (B, U1 - 1)).astype(np.int32)
    lab_d, tl_d, ul_d, off_d = dv(dev, labels), dv(dev, np.asarray(tl, np.int32)), dv(dev, np.asarray(ul, np.int32)), dv(dev, off)
    row_label = K.rnnt_row_labels(lab_d, ul_d, tl_d, off_d, total, T, V)
    parts = -(-V // 128) * 2
    part = torch.full((total, parts, 2), float("nan"), dtype=torch.float32, device=dev)
    pick = torch.full((total, 2), float("nan"), dtype=torch.float32, device=dev)
    K.gemm(h, W, None, total, V, J, J, V, V, bias=bias, lse=(part, row_label, pick))  # raises TfasrUnsupported if the route is not there
    frames, llp, score = [x.cpu().numpy() for x in K.rnnt_align_stats((part, pick), lab_d, ul_d, tl_d, T, V, cell_off=off_d)]
    logits = K.matmul(h, W, bias=bias)
    fm, _, sm = [x.cpu().numpy() for x in K.rnnt_align(logits, lab_d, ul_d, tl_d, T=T, cell_off=off_d)]
    x = logits.double()
    lp = x - torch.logsumexp(x, 1, keepdim=True)
    rl = row_label.long().clamp(min=0)
    blank_all, truth_all = lp[:, 0].cpu().numpy(), lp.gather(1, rl[:, None])[:, 0].cpu().numpy()
    xmax = float(x.abs().max())
    same = 0
    for b in range(B):
        Tl, Ul = tl[b], ul[b]
        bl = blank_all[off[b]:off[b + 1]].reshape(Tl, Ul + 1)
        tr = truth_all[off[b]:off[b + 1]].reshape(Tl, Ul + 1)
        f = frames[b]
        assert (f[Ul:] == -1).all() and (f[:Ul] >= 0).all() and (f[:Ul] < Tl).all() and (np.diff(f[:Ul]) >= 0).all()
        mine, _ = rnnt_path_score(bl, tr, Tl, Ul, f)
        _, _, opt = rnnt_oracle(bl, tr, Tl, Ul, U1 - 1)
        tol = (Tl + Ul + 1) * 2.0 ** -8 * xmax
        print(f"stats-only b={b} Tl={Tl} Ul={Ul}: optimum - path {opt - mine:.3e}, |score - path| {abs(float(score[b]) - mine):.3e}, tol {tol:.3e}")
        assert opt - mine <= tol and abs(float(score[b]) - mine) <= tol and abs(float(score[b]) - float(sm[b])) <= tol
        same += np.array_equal(f, fm[b])
    print(f"stats-only: {same}/{B} utterances with the frames of the materialised route")


# ------------------------------------------------------------------------------------------------------------------ 8. against the loss
def test_transducer_score_is_bracketed_by_the_loss(dev):
    """The best path cannot beat the sum over all C(Tl-1+Ul, Ul) paths, nor fall below their average.  tol: the loss walks Tl+Ul
    diagonals with one f32 two-term log-sum-exp each (hardware exp2 / log2, 1 ulp each, plus the additions): 4 ulp of the running
    value per diagonal, bounded by |cost|; the walk's own additions are inside the same bound."""
    rng = np.random.default_rng(5)
    for B, T, U1, V in ((8, 20, 6, 16), (32, 250, 65, 40)):
        tl, ul = _ragged(rng, B, T, U1 - 1)
        logits = dv(dev, (rng.standard_normal((B, T, U1, V)) * 2).astype(np.float32))
        labels = dv(dev, rng.integers(1, V, (B, U1 - 1)).astype(np.int32))
        tl_d, ul_d = dv(dev, np.asarray(tl, np.int32)), dv(dev, np.asarray(ul, np.int32))
        frames, llp, score_d = [x.clone() for x in K.rnnt_align(logits, labels, ul_d, tl_d)]
        costs, _ = K.rnnt_loss_fwd_bwd(logits, labels, ul_d, tl_d, want_grads=False)
        score, costs = score_d.cpu().numpy().astype(np.float64), costs.cpu().numpy().astype(np.float64)
        for b in range(B):
            tol = 4 * (tl[b] + ul[b] + 1) * 2.0 ** -23 * abs(costs[b])
            npaths = math.comb(tl[b] - 1 + ul[b], ul[b])
            assert score[b] <= -costs[b] + tol, (b, score[b], costs[b], tol)
            assert score[b] >= -costs[b] - math.log(npaths) - tol, (b, score[b], costs[b], npaths, tol)
        # the packed layout holds the same rows: the same walk, bit for bit
        fb, off = [], np.zeros(B + 1, np.int64)
        lg = logits.cpu().numpy()
        for b in range(B):
            fb.append(lg[b, :tl[b], :ul[b] + 1].reshape(-1, V))
            off[b + 1] = off[b] + len(fb[-1])
        fp, lp_, sp = K.rnnt_align(dv(dev, np.concatenate(fb)), labels, ul_d, tl_d, T=T, cell_off=dv(dev, off))
        assert torch.equal(fp, frames) and torch.equal(sp, score_d) and torch.equal(lp_, llp)


def test_ctc_score_is_bracketed_by_the_loss(dev):
    """tol as above with Tl steps of a three-term log-sum-exp (libm expf / logf): 6 ulp of the running value per frame"""
    rng = np.random.default_rng(6)
    for B, T, U, V in ((8, 20, 5, 16), (16, 250, 64, 40)):
        tl, ul = _ragged(rng, B, T, U)
        tl = [max(t, 2 * u + 1) for t, u in zip(tl, ul)]  # every utterance fits, whatever its repeats
        tl = [min(t, T) for t in tl]
        x = (rng.standard_normal((B, T, V)) * 2).astype(np.float32)
        labels = rng.integers(1, V, (B, U)).astype(np.int32)
        logits, lab_d = dv(dev, x), dv(dev, labels)
        tl_d, ul_d = dv(dev, np.asarray(tl, np.int32)), dv(dev, np.asarray(ul, np.int32))
        start, end, llp, score = K.ctc_align(logits, lab_d, ul_d, tl_d)
        costs, _ = K.ctc_loss_fwd_bwd(logits, lab_d, ul_d, tl_d, want_grads=False)
        score, costs = score.cpu().numpy().astype(np.float64), costs.cpu().numpy().astype(np.float64)
        x64 = x.astype(np.float64)
        lp = x64 - (x64.max(-1, keepdims=True) + np.log(np.exp(x64 - x64.max(-1, keepdims=True)).sum(-1, keepdims=True)))
        start, end = start.cpu().numpy(), end.cpu().numpy()
        for b in range(B):
            _, _, _, opt, npaths = ctc_oracle(lp[b], labels[b], tl[b], ul[b], U, 0)
            if npaths == 0:
                assert score[b] == NEG
                continue
            tol = 6 * tl[b] * 2.0 ** -23 * abs(costs[b])
            assert score[b] <= -costs[b] + tol, (b, score[b], costs[b], tol)
            assert score[b] >= -costs[b] - math.log(npaths) - tol, (b, score[b], costs[b], npaths, tol)
            mine, terms = ctc_path_score(lp[b], labels[b], tl[b], ul[b], 0, start[b], end[b])
            ptol = 2 * tl[b] * 2.0 ** -23 * float(np.abs(terms).sum())
            assert opt - mine <= ptol and abs(score[b] - mine) <= ptol, (b, opt, mine, score[b], ptol)


# ------------------------------------------------------------------------------------------------------------------ CTC model
def test_ctc_model_align_end_to_end(dev):
    cfg = configs.conformer_tiny(head="ctc")
    model = ConformerCTC(cfg, dev, dtype=torch.float32, seed=2)
    with torch.no_grad():
        model.ps.p("dec/logits/w").mul_(3.0)
    model.ps.refresh_shadow()
    lens, ulens, U = [4000, 4000, 2500, 3200], [3, 2, 2, 0], 3
    data, labels = batch(cfg.vocab_size, lens, ulens, U, seed=9)
    labels[0, :3] = [5, 5, 7]  # a repeat: needs a blank between
    data = TrainData(data.inputs, TrainLabel(torch.from_numpy(labels), data.labels.labels_length))
    out = model.align(data)
    assert isinstance(out, AlignOutput) and out.ends is not None
    res = model(data.inputs)
    x = res.logits.double().cpu().numpy()
    lp = x - (x.max(-1, keepdims=True) + np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)))
    tl = [min(int(v), x.shape[1]) for v in res.logits_length.tolist()]
    start, end, score = out.frames.cpu().numpy(), out.ends.cpu().numpy(), out.scores.cpu().numpy()
    for b, Ul in enumerate(ulens):
        Tl = tl[b]
        need = Ul + sum(labels[b, u] == labels[b, u + 1] for u in range(Ul - 1))
        assert Tl >= need, "the test's labels must fit the tiny model's frames"
        s, e = start[b], end[b]
        assert (s[Ul:] == -1).all() and (e[Ul:] == -1).all()
        assert all(0 <= s[u] < e[u] <= Tl for u in range(Ul)) and all(e[u] <= s[u + 1] for u in range(Ul - 1))
        if b == 0:
            assert e[0] < s[1]  # the blank between the repeated labels
        mine, terms = ctc_path_score(lp[b], labels[b], Tl, Ul, 0, s, e)
        _, _, _, opt, _ = ctc_oracle(lp[b], labels[b], Tl, Ul, U, 0)
        tol = 2 * Tl * 2.0 ** -23 * float(np.abs(terms).sum())
        print(f"ctc align b={b} Tl={Tl} Ul={Ul}: optimum - path {opt - mine:.3e}, |score - path| {abs(float(score[b]) - mine):.3e}, tol {tol:.3e}")
        assert mine <= opt + 1e-12 and opt - mine <= tol and abs(float(score[b]) - mine) <= tol
    assert out.seconds_per_frame == pytest.approx(cfg.time_reduction_factor * cfg.stride_ms / 1000.0)


# ------------------------------------------------------------------------------------------------------------------ 9. the search
def test_alignment_of_the_greedy_transcript_scores_at_least_the_greedy_path(dev):
    model = tiny("conformer", dev, torch.float32, seed=0)
    with torch.no_grad():
        model.ps.p("joint/vocab/b")[0] += 6.0  # the blank bias at which these utterances mix blanks and labels (4: the token buffer fills up)
    model.ps.refresh_shadow()
    lens = [4000, 3200, 2500]
    rng = np.random.default_rng(10)
    sig = np.clip(rng.standard_normal((3, 4000)) * 0.1, -1, 1).astype(np.float32)
    emitted = 0
    for b, n in enumerate(lens):  # one utterance at a time: the single-utterance search, here with one symbol per frame at most
        one = torch.from_numpy(sig[b:b + 1, :n].copy())
        nlen = torch.tensor([n], dtype=I32)
        toks = model.recognize(PredictInput(one, nlen), max_tokens_per_frame=1).tokens.cpu().numpy()[0]
        hyp = [int(v) for v in toks if v != model.blank]
        Ul = len(hyp)
        emitted += Ul
        labels = np.zeros((1, max(Ul, 1)), np.int32)
        labels[0, :Ul] = hyp
        preds = np.concatenate([np.zeros((1, 1), np.int32), labels], 1)
        data = TrainData(TrainInput(one, nlen, torch.from_numpy(preds), torch.tensor([Ul + 1], dtype=I32)),
                         TrainLabel(torch.from_numpy(labels), torch.tensor([Ul], dtype=I32)))
        out = model.align(data)
        check_transducer_alignment(model, data, labels, [Ul], out, "f32")
        bl, tr, tl, x = f64_lattice(model, data, labels)
        # re-walk the search from its tokens on the f64 logits: every frame takes one decision, a label or a blank, and is left
        u, f = 0, []
        for t in range(tl[0]):
            if u < Ul and int(np.argmax(x[0, t, u])) != model.blank:
                f.append(t)
                u += 1
        assert u == Ul, "the oracle's greedy walk must reproduce the transcript"
        greedy, terms = rnnt_path_score(bl[0], tr[0], tl[0], Ul, f)
        tol = 2 * (tl[0] + Ul + 1) * 2.0 ** -23 * float(np.abs(terms).sum())
        score = float(out.scores[0])
        print(f"greedy b={b}: transcript {hyp} at frames {f}, its path {greedy:.6f}, aligned {out.frames[0, :Ul].tolist()} score {score:.6f}")
        assert score >= greedy - tol, (b, score, greedy)
    assert emitted > 0, "the search emitted nothing: the case shows nothing"


# ------------------------------------------------------------------------------------------------------------------ 10. determinism
def test_deterministic_at_the_bench_shape(dev):
    B, T, U1, V = 32, 250, 65, 1000
    g = torch.Generator(device=dev).manual_seed(3)
    logits = (torch.randn(B, T, U1, V, generator=g, device=dev) * 2).to(torch.bfloat16)
    labels = torch.randint(1, V, (B, U1 - 1), generator=g, device=dev, dtype=I32)
    tl = torch.randint(1, T + 1, (B,), generator=g, device=dev, dtype=I32)
    ul = torch.randint(0, U1, (B,), generator=g, device=dev, dtype=I32)
    a = K.rnnt_align(logits, labels, ul, tl)
    a = [x.clone() for x in a]
    b = K.rnnt_align(logits, labels, ul, tl)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.isfinite(a[2]).all()
    lg = logits[:, :, 0].float().contiguous()  # [B, T, V]
    c = [x.clone() for x in K.ctc_align(lg, labels, ul, torch.maximum(tl, 2 * ul + 1).clamp(max=T))]
    d = K.ctc_align(lg, labels, ul, torch.maximum(tl, 2 * ul + 1).clamp(max=T))
    assert all(torch.equal(x, y) for x, y in zip(c, d))
    assert torch.isfinite(c[3]).all()
