"""tensorflowasr_amd.lm.NGramLM: ARPA reading against hand-computed numbers, the estimator's normalisation, next_state, and the flat
tables: `walk` (the searches' float32 loop) against the float64 model."""
import math

import numpy as np
import pytest

import ctc_lm_oracle as O
from tensorflowasr_amd.lm import LN10, NGramLM

ARPA = """\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-0.7\t1\t-0.3
-0.9\t2\t-0.2
-1.2\t3

\\2-grams:
-0.4\t<s> 1\t-0.1
-0.6\t1 2\t-0.25
-0.8\t2 1
-0.3\t2 </s>

\\3-grams:
-0.2\t<s> 1 2
-0.5\t1 2 1

\\end\\
"""


@pytest.fixture()
def arpa(tmp_path):
    p = tmp_path / "toy.arpa"
    p.write_text(ARPA)
    return NGramLM.from_arpa(str(p), vocab_size=5, blank=0)


def test_arpa_values_equal_hand_computed_numbers(arpa):
    lm = arpa
    assert lm.order == 3 and lm.has_bos and lm.has_eos and (lm.bos, lm.eos) == (5, 6)
    assert lm.log_prob([lm.bos], 1) == pytest.approx(-0.4 * LN10)
    assert lm.log_prob([lm.bos, 1], 2) == pytest.approx(-0.2 * LN10)
    assert lm.log_prob([1, 2], 1) == pytest.approx(-0.5 * LN10)
    # a backed-off trigram: "1 2 3" is not there -> bow(1 2) + "2 3" is not there -> bow(2) + p(3)
    assert lm.log_prob([1, 2], 3) == pytest.approx((-0.25 - 0.2 - 1.2) * LN10)
    # "2 1 2": the context "2 1" has no backoff weight (0), "1 2" is a bigram
    assert lm.log_prob([2, 1], 2) == pytest.approx(-0.6 * LN10)
    # an unseen context costs nothing
    assert lm.log_prob([3, 3], 2) == pytest.approx(-0.9 * LN10)
    # the end of a sentence: "1 2 </s>" -> bow(1 2) + "2 </s>"
    assert lm.log_prob([1, 2], lm.eos) == pytest.approx((-0.25 - 0.3) * LN10)
    # score chains them from <s>
    assert lm.score([1, 2, 1]) == pytest.approx((-0.4 - 0.2 - 0.5) * LN10)
    assert lm.score([1, 2], eos=True) == pytest.approx((-0.4 - 0.2 - 0.25 - 0.3) * LN10)


def test_missing_unigram_takes_unk_log10(tmp_path, arpa):
    assert arpa.log_prob([], 4) == pytest.approx(-10.0 * LN10)
    assert arpa.log_prob([1, 2], 4) == pytest.approx((-0.25 - 0.2 - 10.0) * LN10)
    p = tmp_path / "toy.arpa"
    p.write_text(ARPA)
    lm = NGramLM.from_arpa(str(p), vocab_size=5, blank=0, unk_log10=-3.5)
    assert lm.log_prob([], 4) == pytest.approx(-3.5 * LN10)
    assert all(np.isfinite(lm.log_prob(c, t)) for c in ([], [1], [1, 2], [4, 4]) for t in (1, 2, 3, 4))


def test_vocab_mapping_and_absent_sentence_marks(tmp_path):
    p = tmp_path / "words.arpa"
    p.write_text("\\data\\\nngram 1=2\nngram 2=1\n\n\\1-grams:\n-0.5\ta\t-0.1\n-0.6\tb\n\n\\2-grams:\n-0.2\ta b\n\n\\end\\\n")
    lm = NGramLM.from_arpa(str(p), vocab={"a": 2, "b": 1}, vocab_size=3, blank=0)
    assert not lm.has_bos and not lm.has_eos and lm.order == 2
    assert lm.log_prob([2], 1) == pytest.approx(-0.2 * LN10)
    assert lm.log_prob([1], 2) == pytest.approx(-0.5 * LN10)
    t = lm.tables(1.0, 0.0)
    assert t.start == 0 and t.eos == -1


def test_arpa_files_are_read_as_utf8(tmp_path):
    p = tmp_path / "pieces.arpa"
    p.write_bytes("\\data\\\nngram 1=2\n\n\\1-grams:\n-0.5\t\u2581h\u00e9\n-0.6\t\u00fc\n\n\\end\\\n".encode("utf-8"))
    lm = NGramLM.from_arpa(str(p), vocab={"\u2581h\u00e9": 1, "\u00fc": 2}, vocab_size=3, blank=0)
    assert lm.log_prob([], 1) == pytest.approx(-0.5 * LN10) and lm.log_prob([], 2) == pytest.approx(-0.6 * LN10)


def test_a_file_scoring_the_blank_is_refused(tmp_path):
    p = tmp_path / "blank.arpa"
    p.write_text(ARPA)
    with pytest.raises(ValueError, match="blank"):
        NGramLM.from_arpa(str(p), vocab_size=5, blank=2)


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_estimator_normalises_for_seen_and_unseen_contexts(order):
    V, blank = 7, 3
    lm = O.markov_lm(V, blank, order, seed=4)
    toks = [t for t in range(V) if t != blank]
    rng = np.random.default_rng(order)
    contexts = [(), (lm.bos,)] + [g for g in lm.logp if lm.is_context(g)][:60]
    contexts += [tuple(int(t) for t in rng.choice(toks, size=n)) for n in (1, 2, 3, 4, 6) for _ in range(5)]  # mostly unseen
    for ctx in contexts:
        total = sum(math.exp(lm.log_prob(ctx, t)) for t in toks + [lm.eos])
        assert abs(total - 1.0) < 1e-9, (order, ctx, total)


def test_next_state_is_the_longest_suffix_that_is_a_context(arpa):
    lm = arpa
    assert lm.next_state([lm.bos], 1) == (lm.bos, 1)
    assert lm.next_state([lm.bos, 1], 2) == (1, 2)      # "<s> 1 2" is as long as the order: its suffix
    assert lm.next_state([1, 2], 3) == (3,)             # "2 3" is no n-gram
    assert lm.next_state([2], 1) == (2, 1)
    assert lm.next_state([3], 4) == (4,)
    assert lm.next_state([1, 2, 1, 2, 1], 2) == (1, 2)


@pytest.mark.parametrize("order", [1, 2, 3, 5])
def test_walk_reproduces_the_model_on_every_context(order):
    V, blank = 6, 0
    lm = O.markov_lm(V, blank, order, seed=7)
    for alpha, beta in ((1.0, 0.0), (0.45, -0.8), (2.0, 1.5)):
        t = lm.tables(alpha, beta)
        assert lm.tables(alpha, beta) is t  # cached
        assert t.table_size & (t.table_size - 1) == 0 and t.table_size >= 2 * t.nodes
        assert t.depth[0] == 0 and lm.node_seq(0) == ()
        assert t.start == (lm.node_id((lm.bos,)) if order > 1 else 0)
        for n in range(t.nodes):
            seq = lm.node_seq(n)
            assert t.depth[n] == len(seq)
            if not lm.is_context(seq):
                continue
            for c in [c for c in range(V) if c != blank]:
                inc, nxt = NGramLM.walk(t, n, c)
                assert isinstance(inc, np.float32)
                want = alpha * lm.log_prob(seq, c) + beta
                # at most order + 1 terms, each one float32 rounding of a float64 value, and as many rounded partial sums; the
                # backoffs and alpha * ln p are all <= 0, so no term and no partial sum exceeds |want| + 2 |beta|
                assert abs(float(inc) - want) <= (order + 1) * 2.0 ** -23 * (abs(want) + 2 * abs(beta)), (seq, c, inc, want)
                assert lm.node_seq(nxt) == lm.next_state(seq, c), (seq, c)
            if lm.has_eos:
                inc, _ = NGramLM.walk(t, n, t.eos, eos=True)
                want = alpha * lm.log_prob(seq, lm.eos)  # alpha, no beta
                assert abs(float(inc) - want) <= (order + 1) * 2.0 ** -23 * abs(want)


def test_zero_weights_give_exact_zeros():
    lm = O.markov_lm(6, 0, 3, seed=7)
    t = lm.tables(0.0, 0.0)
    for a in (t.wlogp, t.wbow, t.weos):
        assert a.dtype == np.float32 and not a.any()
    inc, _ = NGramLM.walk(t, t.start, 2)
    assert inc == 0.0
