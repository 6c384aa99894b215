"""Float64 textbook restatement of the CTC prefix beam search with n-gram LM shallow fusion (tfasr_ctc_beam_search_lm[_host]), and
the fixtures its tests share.  Hypotheses are label tuples in a dict, probabilities (blank-ending, label-ending) in float64, the LM
score is alpha * ln P_lm + beta per token straight from NGramLM.log_prob (no tables).  Same definition as the library:
  * a hypothesis ranks by log P_ctc(prefix) + lm(prefix); exact ties: the smaller label sequence first;
  * per frame only the K = min(2W, V-1) acoustically best non-blank classes (lp desc, class asc) extend a hypothesis, plus a repeat
    of its own last label and the classes whose extension is itself a hypothesis of the beam;
  * the final order adds alpha * ln P_lm(</s> | prefix) when the model has </s>.
"""
import itertools

import numpy as np

from tensorflowasr_amd.lm import NGramLM


def log_softmax64(x):
    x = np.asarray(x).astype(np.float64)
    return x - np.logaddexp.reduce(x, axis=-1, keepdims=True)


def lm_of(lm, alpha, beta, prefix, memo=None):
    """alpha * ln P_lm(prefix) + beta * len(prefix), from <s> when the model has it (memo: scores of shorter prefixes, reused)"""
    if memo is None:
        return alpha * lm.score(prefix) + beta * len(prefix)
    if not prefix:
        return 0.0
    if prefix not in memo:
        ctx = ([lm.bos] if lm.has_bos else []) + list(prefix[max(len(prefix) - lm.order, 0):-1])
        memo[prefix] = lm_of(lm, alpha, beta, prefix[:-1], memo) + alpha * lm.log_prob(ctx, prefix[-1]) + beta
    return memo[prefix]


def eos_of(lm, alpha, prefix):
    if not lm.has_eos:
        return 0.0
    ctx = ([lm.bos] if lm.has_bos else []) + list(prefix)
    return alpha * lm.log_prob(ctx, lm.eos)


def fused_beam_search(x, Tb, beam_width, blank, lm, alpha, beta):
    """x [T,V] logits of one utterance, Tb frames of it -> [(labels tuple, score, log_prob, lm_score)], best first (the whole final
    beam)"""
    lp_all = log_softmax64(np.asarray(x)[:Tb].astype(np.float32))
    V = np.asarray(x).shape[1]
    W, K = beam_width, min(2 * beam_width, V - 1)
    beams = {(): (0.0, -np.inf)}
    memo = {}
    for t in range(Tb):
        lp = lp_all[t]
        listed = sorted((c for c in range(V) if c != blank), key=lambda c: (-lp[c], c))[:K]
        nxt = {}

        def add(prefix, pb, pnb):
            a, b = nxt.get(prefix, (-np.inf, -np.inf))
            nxt[prefix] = (np.logaddexp(a, pb), np.logaddexp(b, pnb))

        for prefix, (pb, pnb) in beams.items():
            tot = np.logaddexp(pb, pnb)
            add(prefix, tot + lp[blank], pnb + lp[prefix[-1]] if prefix else -np.inf)
            classes = set(listed)
            if prefix:
                classes.add(prefix[-1])
            classes.update(q[-1] for q in beams if q and q[:-1] == prefix)
            for c in classes:
                add(prefix + (c,), -np.inf, (pb if prefix and c == prefix[-1] else tot) + lp[c])
        ranked = sorted(nxt.items(), key=lambda kv: (-(np.logaddexp(*kv[1]) + lm_of(lm, alpha, beta, kv[0], memo)), kv[0]))
        beams = dict(kv for kv in ranked[:W] if np.logaddexp(*kv[1]) > -np.inf)
    out = []
    for prefix, (pb, pnb) in beams.items():
        ac = np.logaddexp(pb, pnb)
        ls = lm_of(lm, alpha, beta, prefix, memo) + eos_of(lm, alpha, prefix)
        out.append((prefix, ac + ls, ac, ls))
    return sorted(out, key=lambda r: (-r[1], r[0]))


def enumerate_fused(x, blank, lm, alpha, beta):
    """every labelling of x [T,V] by brute force over all alignments -> [(labels, score, log_prob, lm_score)], best first"""
    lp = log_softmax64(np.asarray(x).astype(np.float32))
    T, V = lp.shape
    tot = {}
    for path in itertools.product(range(V), repeat=T):
        lab, prev = [], None
        for c in path:
            if c != blank and c != prev:
                lab.append(c)
            prev = c
        k = tuple(lab)
        tot[k] = np.logaddexp(tot.get(k, -np.inf), sum(lp[t, c] for t, c in enumerate(path)))
    out = []
    for k, ac in tot.items():
        ls = lm_of(lm, alpha, beta, k) + eos_of(lm, alpha, k)
        out.append((k, ac + ls, ac, ls))
    return sorted(out, key=lambda r: (-r[1], r[0]))


# ---------------------------------------------------------------------------------------------------------- fixtures
_LMS = {}


def markov_lm(V, blank, order, seed=0, nseq=None):
    """NGramLM.estimate over token sequences drawn from a seeded first-order Markov chain with a few strongly preferred successors per
    token (so that the model has opinions); cached."""
    key = (V, blank, order, seed, nseq)
    if key not in _LMS:
        rng = np.random.default_rng(1000 * seed + V)
        toks = [t for t in range(V) if t != blank]
        n = len(toks)
        fav = {t: rng.choice(n, size=min(3, n), replace=False) for t in range(n)}
        seqs = []
        for _ in range(nseq or (40 if V > 100 else 80)):
            L = int(rng.integers(1, 13))
            cur = int(rng.integers(n))
            s = [toks[cur]]
            for _ in range(L - 1):
                cur = int(rng.choice(fav[cur])) if rng.random() < 0.8 else int(rng.integers(n))
                s.append(toks[cur])
            seqs.append(s)
        _LMS[key] = NGramLM.estimate(seqs, order, V, blank)
    return _LMS[key]


def chain_lm_score(tables, tokens):
    """what the library reports as lm_score: the chained np.float32 sum of NGramLM.walk from `start`, plus the end-of-sentence term"""
    s, st = np.float32(0.0), tables.start
    for c in tokens:
        inc, st = NGramLM.walk(tables, st, int(c))
        s = np.float32(s + inc)
    if tables.eos >= 0:
        inc, _ = NGramLM.walk(tables, st, tables.eos, eos=True)
        s = np.float32(s + inc)
    return s


def host_lm(x, lens, tables, beam, blank, top_paths=1):
    """tfasr_ctc_beam_search_lm_host on a numpy [B,T,V] batch -> numpy tokens [B,P,T], lengths, score, log_prob, lm_score [B,P]"""
    import torch

    from tensorflowasr_amd import kernels as K

    out = K.ctc_beam_search_lm_host(torch.from_numpy(np.ascontiguousarray(x, np.float32)), np.asarray(lens, np.int32), tables,
                                    beam_width=beam, top_paths=top_paths, blank_index=blank)
    return [o.numpy() for o in out]
