"""Backoff n-gram language model over the model's token ids, for shallow fusion in the CTC prefix beam search
(kernels.ctc_beam_search_lm / ctc_beam_search_lm_host, ConformerCTC.recognize_beam_lm).  Host side only, pure Python + NumPy.

An NGramLM holds the n-grams of an ARPA file (from_arpa) or of the user's own transcripts (estimate) as tuples of token ids, with
natural-log probabilities and backoff weights in float64.  <s> and </s> have the internal ids vocab_size and vocab_size + 1; the
blank token is never scored.  `tables(alpha, beta)` is the flat float32 form both search routines read (include/tfasr_hip.h,
tfasr_ngram_lm_t): alpha and beta are folded in here, so the searches only ADD float32 values, in one fixed order, and the host
routine and the kernel cannot disagree.  `walk` restates that order in NumPy.
"""
import math
from collections import defaultdict

import numpy as np

LN10 = math.log(10.0)
_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _hash(node, token, mask):
    """csrc/beam_trie.h hash(), in 32-bit arithmetic"""
    a = (node * 0x9E3779B1) & 0xFFFFFFFF
    b = (((token + 0x7F4A7C15) & 0xFFFFFFFF) * 0x85EBCA77) & 0xFFFFFFFF
    return (a ^ b) & mask


class NGramTables:
    """tables(alpha, beta) of an NGramLM: NumPy arrays keys [table_size] u64, vals [table_size] i32, wlogp / wbow / weos [nodes] f32,
    suffix / depth [nodes] i32, and the scalars nodes, table_size, order, start, eos; vocab_size and blank say which model's classes
    the token ids are (the searches refuse logits of another V or another blank)."""

    def __init__(self, keys, vals, wlogp, wbow, weos, suffix, depth, order, start, eos, alpha, beta, vocab_size, blank):
        self.keys, self.vals, self.wlogp, self.wbow, self.weos, self.suffix, self.depth = keys, vals, wlogp, wbow, weos, suffix, depth
        self.nodes, self.table_size = int(wlogp.shape[0]), int(keys.shape[0])
        self.order, self.start, self.eos = int(order), int(start), int(eos)
        self.alpha, self.beta = float(alpha), float(beta)
        self.vocab_size, self.blank = int(vocab_size), int(blank)
        self._struct = None   # host tfasr_ngram_lm_t
        self._device = {}     # str(device) -> (tensors, tfasr_ngram_lm_t)

    def child(self, node, token):
        """the node of `node`'s sequence followed by token, or -1: the probe sequence of csrc/beam_trie.h lookup()"""
        mask = self.table_size - 1
        key = np.uint64((int(node) << 32) | int(token))
        h = _hash(int(node), int(token), mask)
        for _ in range(self.table_size):
            k = self.keys[h]
            if k == key:
                return int(self.vals[h])
            if k == _EMPTY:
                return -1
            h = (h + 1) & mask
        return -1


class NGramLM:
    def __init__(self, order, vocab_size, blank, logp, bow):
        """logp: {tuple of ids: ln p} for every n-gram, bow: {tuple: ln backoff} (missing: 0).  Use from_arpa or estimate."""
        self.order, self.vocab_size, self.blank = int(order), int(vocab_size), int(blank)
        self.bos, self.eos = self.vocab_size, self.vocab_size + 1
        self.logp, self.bow = dict(logp), dict(bow)
        if self.order < 1:
            raise ValueError("NGramLM: order < 1")
        if not 0 <= self.blank < self.vocab_size:
            raise ValueError(f"NGramLM: blank {self.blank} outside [0, vocab_size = {self.vocab_size})")
        for g in self.logp:
            if not 1 <= len(g) <= self.order:
                raise ValueError(f"NGramLM: n-gram {g} longer than the order {self.order}")
            if self.blank in g:
                raise ValueError(f"NGramLM: the n-gram {g} scores the blank token {self.blank}; the blank is never scored")
            if len(g) > 1 and g[:-1] not in self.logp:
                raise ValueError(f"NGramLM: n-gram {g} without its prefix {g[:-1]}")
        for t in range(self.vocab_size):
            if t != self.blank and (t,) not in self.logp:
                raise ValueError(f"NGramLM: token {t} has no unigram (every lookup must end at the unigram level)")
        self.has_bos, self.has_eos = (self.bos,) in self.logp, (self.eos,) in self.logp
        self._tables = {}
        self._nodes = None

    # ------------------------------------------------------------------------------------------------ construction
    @classmethod
    def from_arpa(cls, path, vocab=None, vocab_size=None, blank=0, unk_log10=-10.0):
        """Read the ARPA text format (log10 values, optional backoff column, `\\N-grams:` sections).  vocab: {word: token id}; by default
        the words are decimal token ids.  <s> / </s> (either may be absent) get the ids vocab_size / vocab_size + 1.  A non-blank token
        without a unigram gets unk_log10 with backoff 0, so every lookup ends at the unigram level and nothing is -inf.  A file that
        scores the blank token is refused."""
        if vocab_size is None:
            raise ValueError("from_arpa: vocab_size is required")
        vocab_size, blank = int(vocab_size), int(blank)

        def word_id(w):
            if w == "<s>":
                return vocab_size
            if w == "</s>":
                return vocab_size + 1
            if vocab is not None:
                if w not in vocab:
                    raise ValueError(f"from_arpa: word {w!r} is not in the vocabulary mapping")
                t = int(vocab[w])
            else:
                try:
                    t = int(w)
                except ValueError:
                    raise ValueError(f"from_arpa: word {w!r} is not a decimal token id (pass vocab=)") from None
            if not 0 <= t < vocab_size:
                raise ValueError(f"from_arpa: token id {t} of word {w!r} outside [0, {vocab_size})")
            if t == blank:
                raise ValueError(f"from_arpa: the file scores the blank token {blank} (word {w!r}); the blank is never scored")
            return t

        logp, bow, n, order = {}, {}, 0, 0
        with open(path, encoding="utf-8") as f:
            for line in f:
                line = line.strip()
                if not line or line == "\\data\\":
                    continue
                if line == "\\end\\":
                    break
                if line.startswith("ngram ") and "=" in line:
                    if int(line.split("=")[1]) > 0:
                        order = max(order, int(line[6:].split("=")[0]))
                    continue
                if line.startswith("\\") and line.endswith("-grams:"):
                    n = int(line[1:-7])
                    continue
                if n == 0:
                    continue
                parts = line.split()
                if len(parts) not in (n + 1, n + 2):
                    raise ValueError(f"from_arpa: malformed {n}-gram line {line!r}")
                if "<unk>" in parts[1 : n + 1] and (vocab is None or "<unk>" not in vocab):
                    continue  # no token stands for the unknown word: its n-grams can never be asked for
                g = tuple(word_id(w) for w in parts[1 : n + 1])
                logp[g] = float(parts[0]) * LN10
                if len(parts) == n + 2:
                    bow[g] = float(parts[n + 1]) * LN10
                order = max(order, n)
        for t in range(vocab_size):
            if t != blank and (t,) not in logp:
                logp[(t,)] = float(unk_log10) * LN10
        return cls(max(order, 1), vocab_size, blank, logp, bow)

    @classmethod
    def estimate(cls, sequences, order, vocab_size, blank, discount=0.75):
        """Interpolated absolute discounting over token sequences, stored in backoff form.  <s> is the context at a sequence start,
        </s> is counted at its end; the unigram level is interpolated with the uniform distribution over the non-blank tokens.  For
        every context, seen or not, the probabilities over the non-blank tokens and </s> sum to 1."""
        order, vocab_size, blank, D = int(order), int(vocab_size), int(blank), float(discount)
        if order < 1 or not 0.0 < D < 1.0:
            raise ValueError("estimate: order >= 1 and 0 < discount < 1")
        bos, eos = vocab_size, vocab_size + 1
        counts = [defaultdict(int) for _ in range(order + 1)]  # counts[k][k-gram]
        nseq = 0
        for seq in sequences:
            seq = [int(t) for t in seq]
            for t in seq:
                if not 0 <= t < vocab_size or t == blank:
                    raise ValueError(f"estimate: token {t} is the blank or outside [0, {vocab_size})")
            padded = [bos] + seq + [eos]
            nseq += 1
            for k in range(1, order + 1):
                for i in range(len(padded) - k + 1):
                    if k == 1 and padded[i] == bos:
                        continue  # <s> is a context, never a prediction
                    counts[k][tuple(padded[i : i + k])] += 1
        if nseq == 0:
            raise ValueError("estimate: no sequences")
        tokens = [t for t in range(vocab_size) if t != blank]
        uniform = 1.0 / len(tokens)
        # per context h: total count and number of distinct continuations
        total = [defaultdict(int) for _ in range(order)]
        types = [defaultdict(int) for _ in range(order)]
        for k in range(1, order + 1):
            for g, c in counts[k].items():
                total[k - 1][g[:-1]] += c
                types[k - 1][g[:-1]] += 1
        prob = {}  # full interpolated probabilities of the stored n-grams
        gamma = {h: D * types[len(h)][h] / total[len(h)][h] for k in range(order) for h in total[k]}
        g0 = gamma[()]
        for t in tokens:
            prob[(t,)] = max(counts[1].get((t,), 0) - D, 0.0) / total[0][()] + g0 * uniform
        prob[(eos,)] = (counts[1][(eos,)] - D) / total[0][()]
        for k in range(2, order + 1):
            for g, c in sorted(counts[k].items()):
                h = g[:-1]
                prob[g] = (c - D) / total[k - 1][h] + gamma[h] * cls._backoff_prob(prob, gamma, g[1:])
        logp = {g: math.log(p) for g, p in prob.items()}
        bow = {h: math.log(v) for h, v in gamma.items() if h and v > 0.0}
        if order > 1:
            logp[(bos,)] = -99.0 * LN10  # a context only: never looked up as a prediction
        return cls(order, vocab_size, blank, logp, {h: b for h, b in bow.items() if h in logp})

    @staticmethod
    def _backoff_prob(prob, gamma, g):
        """P(g[-1] | g[:-1]) from the levels already filled"""
        w = 1.0
        while g not in prob:
            w *= gamma.get(g[:-1], 1.0)
            g = g[1:]
        return w * prob[g]

    # ------------------------------------------------------------------------------------------------ host scoring (float64)
    def _check_token(self, token):
        token = int(token)
        if token == self.blank or not (0 <= token < self.vocab_size or (token == self.eos and self.has_eos)):
            raise ValueError(f"NGramLM: token {token} is the blank, or neither a vocabulary token nor </s>")
        return token

    def log_prob(self, context, token):
        """ln P(token | context) by backoff; context: token ids (may start with lm.bos), token: a non-blank id or lm.eos"""
        token = self._check_token(token)
        ctx = tuple(int(t) for t in context)
        ctx = ctx[max(len(ctx) - (self.order - 1), 0):] if self.order > 1 else ()
        acc = 0.0
        while ctx + (token,) not in self.logp:
            acc += self.bow.get(ctx, 0.0)
            ctx = ctx[1:]
        return acc + self.logp[ctx + (token,)]

    def score(self, tokens, bos=True, eos=False):
        """ln P of a token sequence: the sum of log_prob over its tokens, from <s> (when the model has one and bos) and, with eos=True,
        the end-of-sentence term"""
        ctx = [self.bos] if (bos and self.has_bos) else []
        s = 0.0
        for t in tokens:
            s += self.log_prob(ctx, t)
            ctx.append(int(t))
        if eos and self.has_eos:
            s += self.log_prob(ctx, self.eos)
        return s

    def is_context(self, seq):
        """a context (state) of the model: the empty sequence, or a stored n-gram shorter than the order that does not end a sentence"""
        seq = tuple(seq)
        return not seq or (len(seq) < self.order and seq in self.logp and seq[-1] != self.eos)

    def next_state(self, context, token):
        """the longest suffix of context + (token,) that is itself a context of the model, as a tuple"""
        g = tuple(int(t) for t in context) + (int(token),)
        g = g[max(len(g) - (self.order - 1), 0):] if self.order > 1 else ()
        while not self.is_context(g):
            g = g[1:]
        return g

    # ------------------------------------------------------------------------------------------------ the flat form
    def _node_list(self):
        if self._nodes is None:
            seqs = [()] + sorted(self.logp, key=lambda g: (len(g), g))
            self._nodes = (seqs, {g: i for i, g in enumerate(seqs)})
        return self._nodes

    def node_seq(self, node):
        return self._node_list()[0][node]

    def node_id(self, seq):
        return self._node_list()[1][tuple(seq)]

    def tables(self, alpha=0.5, beta=0.0):
        """-> NGramTables, cached per (alpha, beta).  Node 0 is the empty context, the other nodes the model's n-grams; wlogp =
        float32(alpha * ln p + beta), wbow = float32(alpha * ln backoff), weos = float32(alpha * ln p) on the </s> entries (the end of a
        sentence takes alpha but no beta); suffix = the node of the sequence without its first token (the longest proper suffix that
        is a node, should a file leave that one out); start = the <s> node when it is a context, else 0."""
        key = (float(alpha), float(beta))
        if key in self._tables:
            return self._tables[key]
        alpha, beta = key
        seqs, ids = self._node_list()
        n = len(seqs)
        cap = 64
        while cap < 2 * n:
            cap <<= 1
        keys = np.full(cap, _EMPTY, np.uint64)
        vals = np.zeros(cap, np.int32)
        wlogp, wbow, weos = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        suffix, depth = np.zeros(n, np.int32), np.zeros(n, np.int32)
        mask = cap - 1
        for i, g in enumerate(seqs):
            if not g:
                continue
            depth[i] = len(g)
            s = g[1:]
            while s not in ids:
                s = s[1:]
            suffix[i] = ids[s]
            lp = self.logp[g]
            if g[-1] == self.eos:
                weos[i] = np.float32(alpha * lp)
            else:
                wlogp[i] = np.float32(alpha * lp + beta)
            wbow[i] = np.float32(alpha * self.bow.get(g, 0.0))
            par, tok = ids[g[:-1]], g[-1]
            h = _hash(par, tok, mask)
            while keys[h] != _EMPTY:
                h = (h + 1) & mask
            keys[h] = np.uint64((par << 32) | tok)
            vals[h] = i
        start = ids[(self.bos,)] if (self.has_bos and self.order > 1) else 0
        t = NGramTables(keys, vals, wlogp, wbow, weos, suffix, depth, self.order, start, self.eos if self.has_eos else -1, alpha, beta,
                        self.vocab_size, self.blank)
        self._tables[key] = t
        return t

    @staticmethod
    def walk(tables, state, token, eos=False):
        """The searches' loop with np.float32 adds -> (increment, next state):
            acc = 0;  while (state, token) has no child: acc += wbow[state], state = suffix[state];  inc = acc + wlogp[child];
            next = child when depth[child] < order, else suffix[child].
        eos=True reads weos instead of wlogp (token = tables.eos: the end-of-sentence term)."""
        t = tables
        acc = np.float32(0.0)
        state = int(state)
        child = t.child(state, token)
        while child < 0:
            if state == 0:
                raise KeyError(f"token {token} has no unigram")
            acc = np.float32(acc + t.wbow[state])
            state = int(t.suffix[state])
            child = t.child(state, token)
        inc = np.float32(acc + (t.weos if eos else t.wlogp)[child])
        return inc, (child if t.depth[child] < t.order else int(t.suffix[child]))
