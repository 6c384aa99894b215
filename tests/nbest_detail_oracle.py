"""NumPy f64 restatement of tfasr_row_lse_entropy and tfasr_ctc_nbest_align (include/tfasr_hip.h): the frame statistics, the Viterbi walk
over the extended label sequence with its tie rule, the spans, the summed log-probabilities and the mean entropies.  Plain loops, no
kernel structure: tests/test_nbest_detail_oracle.py pins it by brute force over every alignment of small cases."""
import json
import os

import numpy as np

NEG = -np.inf
PARITY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "nbest_detail_parity.json")


def write_parity(section, figures):
    """merge one test's measured errors and bounds into profiles/nbest_detail_parity.json"""
    doc = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as f:
            doc = json.load(f)
    doc["what"] = ("max |device - float64| of the parent's kernels and of the n-best detail path on the same inputs; every bound is twice the "
                   "parent's error (tests/test_nbest_align_gpu.py, tests/test_nbest_detailed_gpu.py)")
    doc[section] = figures
    os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
    with open(PARITY_FILE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def frame_stats(x):
    """x [..., V] -> (lse [...], entropy [...]) in f64.  entropy = log(sum e) + sum e (max - x) / sum e with e = exp(x - max); a class
    whose e is 0 (a logit of -inf, or one the caller flushed) contributes 0."""
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    d = x - m
    e = np.exp(d)
    s = e.sum(-1)
    a = np.where(e > 0, -e * np.where(e > 0, d, 0.0), 0.0).sum(-1)
    return m[..., 0] + np.log(s), np.log(s) + a / s


def extended(labels, blank):
    ext = [blank]
    for c in labels:
        ext += [int(c), blank]
    return ext


def moves(ext, s, blank):
    """predecessors of state s, smallest move first"""
    out = [s]
    if s >= 1:
        out.append(s - 1)
    if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
        out.append(s - 2)
    return out


def viterbi(lp, labels, blank):
    """lp [T, V] f64 log-probabilities, labels: ints in [0, V) -> (start [U], end [U], score); a label sequence that does not fit, or
    T == 0: (-1s, -1s, -inf).  A tie takes the smallest move (stay, s-1, s-2), and the final blank at the end."""
    lp = np.asarray(lp, np.float64)
    T, U = lp.shape[0], len(labels)
    none = (np.full(U, -1), np.full(U, -1), NEG)
    if T == 0:
        return none
    ext = extended(labels, blank)
    S = len(ext)
    v = np.full((T, S), NEG)
    mv = np.zeros((T, S), np.int64)
    for s in range(min(S, 2)):
        v[0, s] = lp[0, ext[s]]
    for t in range(1, T):
        for s in range(S):
            best, arg = NEG, 0
            for k, q in enumerate(moves(ext, s, blank)):
                if k == 0 or v[t - 1, q] > best:
                    best, arg = v[t - 1, q], k
            v[t, s] = best + lp[t, ext[s]]
            mv[t, s] = arg
    a1, a2 = v[T - 1, S - 1], (v[T - 1, S - 2] if S >= 2 else NEG)
    score = max(a1, a2)
    if score == NEG:
        return none
    s = S - 2 if a2 > a1 else S - 1
    states = [0] * T
    for t in range(T - 1, -1, -1):
        states[t] = s
        if t > 0:
            s -= mv[t, s]
    return spans(states, U) + (score,)


def spans(states, U):
    """[start, end) of every label along a state path: the first frame and one past the last frame spent in its state"""
    start, end = np.full(U, -1), np.full(U, -1)
    for t, s in enumerate(states):
        if s & 1:
            u = s >> 1
            if start[u] < 0:
                start[u] = t
            end[u] = t + 1
    return start, end


def label_sums(lp, labels, start, end):
    out = np.zeros(len(labels))
    for u, c in enumerate(labels):
        if start[u] >= 0:
            out[u] = sum(lp[t, int(c)] for t in range(start[u], end[u]))
    return out


def mean_entropy(frame_ent, start, end):
    out = np.zeros(len(start))
    for u in range(len(start)):
        if start[u] >= 0:
            out[u] = sum(frame_ent[t] for t in range(start[u], end[u])) / (end[u] - start[u])
    return out


def align_row(lp, frame_ent, labels, blank):
    """one hypothesis against one utterance's log-probabilities -> (start, end, label_lp, label_entropy, score)"""
    V = lp.shape[1]
    labels = [min(max(int(c), 0), V - 1) for c in labels]
    start, end, score = viterbi(lp, labels, blank)
    return start, end, label_sums(lp, labels, start, end), mean_entropy(frame_ent, start, end), score


def nbest_align(logits, logit_len, labels, label_len, blank, U=None):
    """tfasr_ctc_nbest_align: logits [B, T, V], labels [B, P, W], label_len [B, P] -> (start, end [B, P, U] int, label_lp, label_entropy
    [B, P, U] f64, score [B, P] f64).  label_len < 0 or > U: a dead row."""
    logits = np.asarray(logits, np.float64)
    B, T, V = logits.shape
    P, W = labels.shape[1], labels.shape[2]
    U = W if U is None else U
    lse, ent = frame_stats(logits)
    start, end = np.full((B, P, U), -1), np.full((B, P, U), -1)
    lab_lp, lab_ent, score = np.zeros((B, P, U)), np.zeros((B, P, U)), np.full((B, P), NEG)
    for b in range(B):
        Tl = min(int(logit_len[b]), T)
        lp = logits[b, :max(Tl, 0)] - lse[b, :max(Tl, 0), None]
        for p in range(P):
            n = int(label_len[b, p])
            if n < 0 or n > U:
                continue
            s, e, a, h, sc = align_row(lp, ent[b], labels[b, p, :n], blank)
            start[b, p, :n], end[b, p, :n], lab_lp[b, p, :n], lab_ent[b, p, :n], score[b, p] = s, e, a, h, sc
    return start, end, lab_lp, lab_ent, score
