"""Tokenizer.word_spans: which tokens spell which word, so that the per-token frames of a forced alignment become word times."""
import os

import numpy as np
import pytest

from tensorflowasr_amd import tokenizers as tk

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "librispeech")
TEXTS = ("the quick brown fox's tail", "HE HOPED there would be stew for dinner", "turnips and carrots  and bruised potatoes", "it's", "a", "")


def check_spans(t, ids, separators):
    """spans are ordered, disjoint and inside the sequence; every token outside a span is a separator; words joined = detokenize"""
    spans = t.word_spans(ids)
    covered = np.zeros(len(ids), bool)
    prev = -1
    for word, a, b in spans:
        assert word and " " not in word
        assert prev < a <= b < len(ids), (spans, len(ids))
        covered[a:b + 1] = True
        prev = b
    assert all(int(i) in separators for i in np.asarray(ids)[~covered]), (spans, ids)
    assert " ".join(w for w, _, _ in spans) == t.detokenize(ids)[0]
    return spans


def test_char_tokenizer_word_spans():
    t = tk.get({"type": "characters", "blank_index": 0, "vocabulary": f"{REF}/characters/english.vocab"})
    space = t.tokens2indices[" "]
    sep = {space, 0, -1}
    for text in TEXTS:
        ids = t.tokenize(text)
        spans = check_spans(t, ids, sep)
        assert [w for w, _, _ in spans] == tk.normalize_text(text).split()
        for w, a, b in spans:  # a span of characters is exactly its word
            assert b - a + 1 == len(w) and "".join(t.tokens[i] for i in ids[a:b + 1]) == w
    ids = t.tokenize("ab cd")
    assert t.word_spans(ids) == [("ab", 0, 1), ("cd", 3, 4)]
    # blanks and -1 padding spell nothing and do not split a word; a leading / doubled space opens no empty word
    padded = np.concatenate([[0, space], ids[:1], [0], ids[1:3], [space], ids[3:], [-1, -1]]).astype(np.int32)
    assert check_spans(t, padded, sep) == [("ab", 2, 4), ("cd", 7, 8)]
    assert t.word_spans(np.zeros(0, np.int32)) == []


def test_sentencepiece_word_spans():
    pytest.importorskip("sentencepiece")
    for name in ("train_bpe_1000", "train_bpe_256"):
        path = f"{REF}/sentencepiece/{name}.model"
        if not os.path.exists(path):
            pytest.skip("no BPE model on this machine")
        t = tk.get({"type": "sentencepiece", "blank_index": 0, "vocabulary": path})
        for text in TEXTS:
            ids = t.tokenize(text)
            spans = check_spans(t, ids, {0, -1})
            assert [w for w, _, _ in spans] == tk.normalize_text(text).split()
            if len(ids):  # in-vocabulary text: the spans tile the token sequence
                assert spans[0][1] == 0 and spans[-1][2] == len(ids) - 1
                assert all(nxt[1] == cur[2] + 1 for cur, nxt in zip(spans, spans[1:]))
        ids = t.tokenize("stew for dinner")
        padded = np.concatenate([ids, [-1, -1]]).astype(np.int32)
        assert t.word_spans(padded) == t.word_spans(ids)


def test_wordpiece_has_no_word_spans():
    t = tk.WordPieceTokenizer.__new__(tk.WordPieceTokenizer)
    with pytest.raises(NotImplementedError):
        t.word_spans([1, 2])
