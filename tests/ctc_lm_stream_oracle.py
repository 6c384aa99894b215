"""Float64 restatement of the fused CTC prefix beam search run chunk by chunk (K.CtcLmBeamStream, tfasr_ctc_beam_lm_*; DESIGN.md 4b-4
"in streaming sessions"), with a prune point after every chunk.

The frame rule is ctc_lm_oracle.fused_beam_search's (a hypothesis ranks by log P_ctc + lm, only the K = min(2W, V-1) acoustically best
non-blank classes extend it, plus a repeat of its last label and the classes whose extension is itself in the beam), stated here as a
function of one frame so that a prune point can stand between two frames; the horizon rule is beam_horizon_oracle.Horizon, unchanged.
What the fusion changes between the frames: at a prune point the rows rank by total + lm WITHOUT the end-of-sentence term (the stream
is still running), and the best row - the one whose path the horizon's target is taken on - is the best in that order, not the
acoustically best; at the end the rows rank WITH the term, the one-shot search's final order.
`ctc_lm_stream` reports every decision margin as beam_horizon_oracle.ctc_stream does (last kept against first dropped candidate of
every frame, best against second-best row at every prune point) and, because the tests compare the live rows in their order, the gaps
between all neighbouring live rows at the prune points and in the final order as well.
"""
import numpy as np

from beam_horizon_oracle import NEG, Horizon, _gap, lcp
from ctc_lm_oracle import eos_of, lm_of, log_softmax64


def fused_frame(beams, lp, blank, W, lm, alpha, beta, memo):
    """one frame: beams {labels: (p_blank, p_label)} -> (the next beam in rank order as [(labels, (pb, pnb))], margin at the cut)"""
    K = min(2 * W, len(lp) - 1)
    listed = sorted((c for c in range(len(lp)) if c != blank), key=lambda c: (-lp[c], c))[:K]
    nxt = {}

    def add(prefix, pb, pnb):
        a, b = nxt.get(prefix, (NEG, NEG))
        nxt[prefix] = (np.logaddexp(a, pb), np.logaddexp(b, pnb))

    for prefix, (pb, pnb) in beams.items():
        tot = np.logaddexp(pb, pnb)
        add(prefix, tot + lp[blank], pnb + lp[prefix[-1]] if prefix else NEG)
        classes = set(listed)
        if prefix:
            classes.add(prefix[-1])
        classes.update(q[-1] for q in beams if q and q[:-1] == prefix)
        for c in classes:
            add(prefix + (c,), NEG, (pb if prefix and c == prefix[-1] else tot) + lp[c])
    key = lambda kv: np.logaddexp(*kv[1]) + lm_of(lm, alpha, beta, kv[0], memo)  # noqa: E731
    ranked = sorted((kv for kv in nxt.items() if np.logaddexp(*kv[1]) > NEG), key=lambda kv: (-key(kv), kv[0]))
    return ranked[:W], _gap([key(kv) for kv in ranked], W)


def _neighbour_gaps(keys):
    return [a - b for a, b in zip(keys, keys[1:])]


def ctc_lm_stream(x, W, blank, C, lm, alpha, beta, H=None, Tcap=None):
    """x [T, V] logits of one stream, a prune point after every C frames (and after the last ones) -> dict(
      steps  = [(frames, committed, [(labels, total + lm)] best first)] per prune point (beam_horizon_oracle.ctc_stream's form),
      parts  = per prune point [(total, lm)] of the same rows,
      final  = [(labels, score, log_prob, lm_score)] of the last beam, best first WITH the end-of-sentence term,
      margin, horizon = the Horizon,
      flips  = the prune points at which the fused-best row is not the acoustically best row).
    Tcap as in ctc_stream: the stream compacts before a chunk that would take its trie's frame count past Tcap."""
    lp_all = log_softmax64(np.asarray(x, np.float32))
    hz, beams, memo = Horizon(H), {(): (0.0, NEG)}, {}
    steps, parts, margins, trie_frames, flips = [], [], [], 0, 0
    tot = lambda y: np.logaddexp(*beams[y])  # noqa: E731
    lmv = lambda y: lm_of(lm, alpha, beta, y, memo)  # noqa: E731
    for t0 in range(0, len(lp_all), C):
        chunk = lp_all[t0:t0 + C]
        if Tcap is not None and trie_frames + len(chunk) > Tcap:
            hz.compact(list(beams))
            trie_frames = max(len(y) for y in beams) - min(len(hz.committed), len(lcp(list(beams))))
        trie_frames += len(chunk)
        assert Tcap is None or trie_frames <= Tcap, "the uncommitted part and the chunk do not fit the trie: a stream would refuse"
        for lp in chunk:
            ranked, gap = fused_frame(beams, lp, blank, W, lm, alpha, beta, memo)
            if gap is not None:
                margins.append(gap)
            hz.grow([y for y, _ in ranked])
            beams = dict(ranked)
        rows = sorted(beams, key=lambda y: (-(tot(y) + lmv(y)), y))
        margins += _neighbour_gaps([tot(y) + lmv(y) for y in rows])
        flips += rows[0] != min(beams, key=lambda y: (-tot(y), y))
        kept = hz.prune(len(chunk), rows)
        beams = {y: beams[y] for y in kept}
        steps.append((hz.now, hz.committed, [(y, float(tot(y) + lmv(y))) for y in kept]))
        parts.append([(float(tot(y)), float(lmv(y))) for y in kept])
    final = []
    for y in beams:
        ls = lmv(y) + eos_of(lm, alpha, y)
        final.append((y, tot(y) + ls, tot(y), ls))
    final.sort(key=lambda r: (-r[1], r[0]))
    margins += _neighbour_gaps([r[1] for r in final])
    return dict(steps=steps, parts=parts, final=final, margin=min(margins, default=np.inf), horizon=hz, flips=flips)


# ---------------------------------------------------------------------------------------------------------- the rule test's inputs
# beam_horizon_oracle.quiet_loud logits [60, 6] with blank 5 under markov_lm(6, 5, 3, seed=3) at (alpha, beta) = RULE_WEIGHTS.  Over
# every (W, H, C, Tcap) of RULE_CASES the smallest oracle margin of these seeds is 2.55e-3, 4.23e-3 and 2.71e-3 (found on the CPU and
# pinned by test_ctc_lm_stream_oracle.py: >= 1e-3).
RULE_SEEDS = (6, 15, 24)
RULE_WEIGHTS = (1.2, -0.6)
RULE_T, RULE_V, RULE_BLANK, RULE_ORDER, RULE_TCAP = 60, 6, 5, 3, 24
RULE_CASES = [(W, H, C, Tcap) for W in (2, 4, 8) for H in (4, 16) for C in (1, 4) for Tcap in (None, RULE_TCAP)]
_RUNS = {}


def rule_inputs():
    from beam_horizon_oracle import quiet_loud
    from ctc_lm_oracle import markov_lm

    x = np.stack([quiet_loud(np.random.default_rng(s), RULE_T, RULE_V, RULE_BLANK) for s in RULE_SEEDS])
    return x, markov_lm(RULE_V, RULE_BLANK, RULE_ORDER, seed=3)


def rule_runs(W, H, C, Tcap):
    """the oracle's runs of the three streams for one case, computed once"""
    key = (W, H, C, Tcap)
    if key not in _RUNS:
        x, lm = rule_inputs()
        _RUNS[key] = [ctc_lm_stream(x[b], W, RULE_BLANK, C, lm, *RULE_WEIGHTS, H=H, Tcap=Tcap) for b in range(len(x))]
    return _RUNS[key]
