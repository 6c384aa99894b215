"""Float64 restatement of the beam streams' commit horizon (tfasr_*_beam_commit_horizon) for both heads.

`Horizon` is the rule alone, on label tuples: it carries the trie's creation order (a sequence gets the next id the first time it is in
a beam; the winners of a frame in rank order, as grow_trie numbers them), the list of prune points (frames consumed, ids handed out) and,
at a prune point `now`, with X = the id count logged at the latest point at or before now - H:
    target = the longest prefix of the best row whose id is < X (it was in the trie H frames ago);
    target longer than the live rows' common prefix -> the rows that do not start with target are removed, committed = target;
    otherwise committed = the common prefix (the plain commit; also when there is no such point, or H is None).
`ctc_stream` / `rnnt_stream` run the two searches frame by frame (the CTC prefix search of ctc_lm_oracle.fused_beam_search without an LM,
the modified transducer search of test_rnnt_beam_gpu.model_oracle) with a prune point after every chunk, and report every decision
margin: last kept against first dropped candidate of every frame, best against second-best row at every prune point.
"""
import numpy as np

from ctc_lm_oracle import log_softmax64

NEG = -np.inf


def lcp(seqs):
    out = []
    for col in zip(*seqs):
        if any(c != col[0] for c in col):
            break
        out.append(col[0])
    return tuple(out)


class Horizon:
    def __init__(self, H=None):
        self.H, self.ids, self.points, self.now, self.committed = H, {(): 0}, [], 0, ()
        self.fired = self.plain = 0  # prune points that removed a row / that left the common prefix in charge
        self.case = []  # per prune point with an X: where the target lay against the common prefix

    def grow(self, seqs):
        """the sequences of a frame's new beam, in rank order"""
        for y in seqs:
            if y not in self.ids:
                assert y[:-1] in self.ids  # a node's parent exists (and has the smaller id)
                self.ids[y] = len(self.ids)

    def prune(self, frames, rows):
        """`frames` more frames were searched; rows = the live label tuples, best first -> the rows that stay (in their order)"""
        assert frames > 0 and rows
        self.now += frames
        self.points.append((self.now, len(self.ids)))
        X = None
        if self.H is not None:
            old = [n for f, n in self.points if f <= self.now - self.H]
            X = old[-1] if old else None
        ca = lcp(rows)
        new, kept = ca, list(rows)
        if X is not None:
            best = rows[0]
            target = max((best[:k] for k in range(len(best) + 1) if self.ids[best[:k]] < X), key=len)
            self.case.append("below" if len(target) > len(ca) else "at" if target == ca else "above")
            if len(target) > len(ca):
                kept = [y for y in rows if y[:len(target)] == target]
                new = target
                self.fired += len(kept) < len(rows)
            else:
                self.plain += 1
        assert all(y[:len(new)] == new for y in kept)  # committed is a prefix of every live row
        if len(new) >= len(self.committed):
            assert new[:len(self.committed)] == self.committed  # and never shrinks
            self.committed = new
        else:
            assert self.committed[:len(new)] == new
        return kept

    def compact(self, rows):
        """what a compaction does to the creation order: only the live rows' prefixes keep their ids (renumbered in order), the logged
        counts become the kept ids below them.  A sequence that is dropped here and wins again later comes back with a NEW id - it
        counts as younger than it is, which is the one way a compaction can change what a horizon does (see
        test_beam_horizon_oracle.test_a_compaction_makes_a_returning_sequence_young)."""
        keep = {y[:k] for y in rows for k in range(len(y) + 1)}
        old = sorted(self.ids.items(), key=lambda kv: kv[1])
        self.points = [(f, sum(1 for y, i in old if y in keep and i < n)) for f, n in self.points]
        self.ids = {y: j for j, y in enumerate(y for y, _ in old if y in keep)}


def quiet_loud(rng, T, V, blank, quiet=0.75):
    """logits [T, V] f32: `quiet` of the frames N(0,1) * 0.5 with +8 on the blank, the rest N(0,1) * 2"""
    x = rng.standard_normal((T, V))
    q = rng.random(T) < quiet
    x = np.where(q[:, None], x * 0.5, x * 2.0)
    x[q, blank] += 8.0
    return x.astype(np.float32)


def _gap(totals, k):
    """margin between the k-th and the (k+1)-th of totals sorted descending (None when there is no (k+1)-th finite one)"""
    return totals[k - 1] - totals[k] if len(totals) > k and totals[k] > NEG else None


def ctc_frame(beams, lp, blank, W):
    """one frame of the prefix search: beams {labels: (p_blank, p_label)} -> (next beams in rank order as a list of (labels, (pb, pnb)),
    margin at the cut or None)"""
    nxt = {}

    def add(prefix, pb, pnb):
        a, b = nxt.get(prefix, (NEG, NEG))
        nxt[prefix] = (np.logaddexp(a, pb), np.logaddexp(b, pnb))

    for prefix, (pb, pnb) in beams.items():
        tot = np.logaddexp(pb, pnb)
        add(prefix, tot + lp[blank], pnb + lp[prefix[-1]] if prefix else NEG)
        for c in range(len(lp)):
            if c != blank:
                add(prefix + (c,), NEG, (pb if prefix and c == prefix[-1] else tot) + lp[c])
    ranked = sorted(nxt.items(), key=lambda kv: (-np.logaddexp(*kv[1]), kv[0]))
    ranked = [kv for kv in ranked if np.logaddexp(*kv[1]) > NEG]
    return ranked[:W], _gap([np.logaddexp(*v) for _, v in ranked], W)


def ctc_stream(x, W, blank, C, H=None, Tcap=None):
    """x [T, V] logits of one stream, a prune point after every C frames (and after the last ones) ->
    dict(steps = [(frames, committed, [(labels, total)] best first)] per prune point, margin, horizon = the Horizon).  Tcap: the stream
    compacts before a chunk that would take its trie's frame count past Tcap (the count restarts at the deepest live row's depth below
    the new root), as a K.CtcBeamStream with that capacity is driven."""
    lp_all = log_softmax64(np.asarray(x, np.float32))
    hz, beams, steps, margins, trie_frames = Horizon(H), {(): (0.0, NEG)}, [], [], 0
    for t0 in range(0, len(lp_all), C):
        chunk = lp_all[t0:t0 + C]
        if Tcap is not None and trie_frames + len(chunk) > Tcap:
            hz.compact(list(beams))
            trie_frames = max(len(y) for y in beams) - min(len(hz.committed), len(lcp(list(beams))))
        trie_frames += len(chunk)
        for lp in chunk:
            ranked, gap = ctc_frame(beams, lp, blank, W)
            if gap is not None:
                margins.append(gap)
            hz.grow([y for y, _ in ranked])
            beams = dict(ranked)
        rows = sorted(beams, key=lambda y: (-np.logaddexp(*beams[y]), y))
        tots = [np.logaddexp(*beams[y]) for y in rows]
        if _gap(tots, 1) is not None:
            margins.append(_gap(tots, 1))
        kept = hz.prune(len(chunk), rows)
        beams = {y: beams[y] for y in kept}
        steps.append((hz.now, hz.committed, [(y, float(np.logaddexp(*beams[y]))) for y in kept]))
    return dict(steps=steps, margin=min(margins, default=np.inf), horizon=hz)


def rnnt_stream(net, ej, W, blank, C, H=None):
    """the transducer counterpart on one utterance's joint encoder projection ej [n, J] (net: test_rnnt_beam_gpu.Net); the beam is kept
    best first, so the best row at a prune point is row 0 -> the dict of ctc_stream"""
    from test_rnnt_beam_gpu import beam_step

    U = net.W["pred/lstm/rk"].shape[0]
    h0 = c0 = np.zeros(U)
    hyps = [dict(seq=(), tot=0.0, tok=blank, h=h0, c=c0, post=net.step(blank, h0, c0))]
    hz, steps, margins = Horizon(H), [], []
    for t0 in range(0, len(ej), C):
        chunk = ej[t0:t0 + C]
        for e in chunk:
            lps = [net.logp(e, hy["post"][2]) for hy in hyps]
            nxt, _, margin = beam_step([(hy["seq"], hy["tot"]) for hy in hyps], lps, blank, W)
            if margin is not None:
                margins.append(margin)
            new = []
            for y, tot, src, lab in nxt:
                if lab < 0:
                    new.append(dict(hyps[src], seq=y, tot=tot))
                else:
                    hp, cp, _ = hyps[src]["post"]
                    new.append(dict(seq=y, tot=tot, tok=lab, h=hp, c=cp, post=net.step(lab, hp, cp)))
            hyps = new
            hz.grow([hy["seq"] for hy in hyps])
        if len(hyps) > 1:
            margins.append(hyps[0]["tot"] - hyps[1]["tot"])
        kept = set(hz.prune(len(chunk), [hy["seq"] for hy in hyps]))
        hyps = [hy for hy in hyps if hy["seq"] in kept]
        steps.append((hz.now, hz.committed, [(hy["seq"], float(hy["tot"])) for hy in hyps]))
    return dict(steps=steps, margin=min(margins, default=np.inf), horizon=hz, hyps=hyps)
