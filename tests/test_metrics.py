"""metrics.py on the host: the edit-distance definition against enumeration of all alignments, the rate formulas, the text encoders,
the results file and the accumulator.  Everything is an integer or a ratio of two: comparisons are exact."""
import math
import random

import numpy as np
import pytest
import torch

from tensorflowasr_amd import metrics as M


def brute_force(h, r):
    """Every alignment of h against r (hit / substitution on a pair, insertion of a hypothesis symbol, deletion of a reference symbol):
    minimum distance, then most hits; the other counts follow from the identity of the module docstring."""
    best = [None]

    def walk(i, j, d, hits):
        if i == len(h) and j == len(r):
            if best[0] is None or (d, -hits) < best[0]:
                best[0] = (d, -hits)
            return
        if i < len(h) and j < len(r):
            walk(i + 1, j + 1, d + (h[i] != r[j]), hits + (h[i] == r[j]))
        if i < len(h):
            walk(i + 1, j, d + 1, hits)
        if j < len(r):
            walk(i, j + 1, d + 1, hits)

    walk(0, 0, 0, 0)
    d, hits = best[0][0], -best[0][1]
    ins = d - (len(r) - hits)
    dele = ins + len(r) - len(h)
    return d, hits, len(r) - hits - dele, dele, ins


def rows(seqs, width, fill):
    out = np.full((len(seqs), width), fill, np.int32)
    for k, s in enumerate(seqs):
        out[k, : len(s)] = s
    return out, np.asarray([len(s) for s in seqs], np.int32)


def table(counts):
    return np.stack([np.asarray(c) for c in counts], 1)


def test_host_routine_equals_enumeration_of_all_alignments():
    rng = random.Random(0)
    hyps = [[rng.randrange(3) for _ in range(rng.randrange(6))] for _ in range(2500)]
    refs = [[rng.randrange(3) for _ in range(rng.randrange(6))] for _ in range(2500)]
    h, hn = rows(hyps, 5, -7)  # what lies past a length must not matter: out-of-alphabet on one side, in-alphabet on the other
    r, rn = rows(refs, 5, 1)
    got = table(M.edit_distance_host(h, r, hn, rn))
    want = np.asarray([brute_force(a, b) for a, b in zip(hyps, refs)])
    np.testing.assert_array_equal(got, want)
    assert got.dtype == np.int32
    assert (got[:, 0] == got[:, 2] + got[:, 3] + got[:, 4]).all()


@pytest.mark.parametrize("hyp, ref, want", [((0, 1), (1, 0), (2, 1, 0, 1, 1)), ((), (1, 2), (2, 0, 0, 2, 0)), ((1,), (), (1, 0, 0, 0, 1))])
def test_tie_rule_examples(hyp, ref, want):
    h, hn = rows([hyp], 2, 0)
    r, rn = rows([ref], 2, 0)
    assert table(M.edit_distance_host(h, r, hn, rn)).tolist() == [list(want)]
    assert brute_force(hyp, ref) == want


def test_compaction_equals_explicit_lengths():
    h = np.array([[0, -1, 5, 3, 0, 0], [0, 0, 0, 0, -1, -1], [4, 4, 0, 9, -1, 2]], np.int32)
    r = np.array([[5, 3, 7, -1], [1, 0, 0, 0], [0, 0, 0, 0]], np.int32)
    hc, hn = rows([[5, 3], [], [4, 4, 9, 2]], 4, 0)
    rc, rn = rows([[5, 3, 7], [1], []], 3, 0)
    want = table(M.edit_distance_host(hc, rc, hn, rn))
    np.testing.assert_array_equal(table(M.edit_distance_host(h, r, skip_id=0)), want)
    np.testing.assert_array_equal(table(M.edit_distance_host(h, rc, None, rn, skip_id=0)), want)
    assert want.tolist() == [[1, 2, 0, 1, 0], [1, 0, 0, 1, 0], [4, 0, 0, 0, 4]]
    keep0 = table(M.edit_distance_host(h, r))  # without a skip id only negative entries are dropped
    assert keep0[1].tolist() == [1, 3, 1, 0, 0]


def test_formulas_on_a_hand_example():
    words = M.ErrorStats().update(M.score_texts(["a x c"], ["a b c d"], "word"))
    assert (words.hits, words.substitutions, words.deletions, words.insertions) == (2, 1, 1, 0)
    assert (words.hyp_length, words.ref_length, words.pairs) == (3, 4, 1)
    assert words.wer == 0.5 and words.mer == 0.5 and words.wip == (2 / 4) * (2 / 3) and words.wil == 1 - (2 / 4) * (2 / 3)
    assert words.wip == pytest.approx(1 / 3) and words.wil == pytest.approx(2 / 3)
    chars = M.score_texts(["a x c"], ["a b c d"], "char")
    assert int(chars.distance[0]) == 3
    assert M.ErrorStats().update(chars).error_rate == 3 / 7


def test_encode_pairs_units():
    h, hn, r, rn = M.encode_pairs(["the  cat   sat", "dog"], ["the cat", "a dog  sat"], "word")
    assert hn.tolist() == [3, 1] and rn.tolist() == [2, 3]  # repeated spaces collapse
    assert h.dtype == np.int32 and r.dtype == np.int32
    the, cat, sat, dog = h[0, 0], h[0, 1], h[0, 2], h[1, 0]
    assert len({int(the), int(cat), int(sat), int(dog)}) == 4
    assert r[0, :2].tolist() == [the, cat] and r[1, 1:3].tolist() == [dog, sat]  # one table for both sides and all rows
    assert int(r[1, 0]) not in (the, cat, sat, dog)
    h, hn, r, rn = M.encode_pairs([" a  b "], ["a b"], "char")
    assert h[0, : hn[0]].tolist() == [ord("a"), 32, 32, ord("b")] and rn.tolist() == [3]  # stripped, inner spaces kept
    _, hn, _, rn = M.encode_pairs(["é"], ["e"], "char")
    assert hn.tolist() == [1]
    h, hn, _, _ = M.encode_pairs(["é"], ["e"], "byte")
    assert hn.tolist() == [2] and h[0, :2].tolist() == [0xC3, 0xA9]
    h, hn, r, rn = M.encode_pairs(["", ""], ["", "x"], "word")
    assert hn.tolist() == [0, 0] and rn.tolist() == [0, 1] and h.shape[1] >= 1
    with pytest.raises(ValueError):
        M.encode_pairs(["a"], ["a"], "phoneme")
    with pytest.raises(ValueError):
        M.encode_pairs(["a"], [], "word")


def test_results_file_round_trip_and_hand_written_file(tmp_path):
    p = tmp_path / "out.tsv"
    refs = ["a b c d", "hello world", ""]
    greedy = ["a x c", "hello world", "uh"]
    beam = ["a b c d", "hello", ""]
    with M.ResultsWriter(str(p)) as w:
        w.write(["u1.flac", "u2.flac"], refs[:2], greedy[:2], beam[:2])
        w.write(["u3.flac"], refs[2:], greedy[2:], beam[2:])
    text = p.read_text().split("\n")
    assert text[0] == "PATH\tGROUND_TRUTH\tGREEDY\tBEAM_SEARCH" and text[1] == "u1.flac\ta b c d\ta x c\ta b c d" and text[3] == "u3.flac\t\tuh\t"
    assert M.read_results(str(p)) == (["u1.flac", "u2.flac", "u3.flac"], refs, greedy, beam)
    got = M.evaluate_hypotheses(str(p))
    assert set(got) == {"greedy", "beam"} and set(got["greedy"]) == {"wer", "cer", "mer", "wil", "wip"}
    for name, hyps in (("greedy", greedy), ("beam", beam)):
        words = M.ErrorStats().update(M.score_texts(hyps, refs, "word"))
        chars = M.ErrorStats().update(M.score_texts(hyps, refs, "char"))
        assert got[name] == M.summary(words, chars)
    # greedy words: S 1 D 1 | hits 2 | I 1 (against the empty reference); 6 reference words, 6 hypothesis words, 4 hits
    assert got["greedy"]["wer"] == 3 / 6 and got["greedy"]["mer"] == 3 / 7 and got["greedy"]["wip"] == (4 / 6) * (4 / 6)
    # greedy characters: "a x c" / "a b c d" 3, "uh" / "" 2, over 7 + 11 reference characters
    assert got["greedy"]["cer"] == 5 / 18
    # beam: one deleted word of 6, " world" = 6 deleted characters of 18
    assert got["beam"] == {"wer": 1 / 6, "cer": 6 / 18, "mer": 1 / 6, "wil": 1 - (5 / 6) * (5 / 5), "wip": (5 / 6) * (5 / 5)}
    q = tmp_path / "hand.tsv"
    q.write_text("PATH\tGROUND_TRUTH\tGREEDY\tBEAM_SEARCH\nx\tone two\tone too\tone two three\n")
    got = M.evaluate_hypotheses(str(q), cer_unit="byte")
    assert got["greedy"] == {"wer": 0.5, "cer": 1 / 7, "mer": 0.5, "wil": 1 - 0.25, "wip": 0.25}
    assert got["beam"] == {"wer": 0.5, "cer": 6 / 7, "mer": 1 / 3, "wil": 1 - (2 / 2) * (2 / 3), "wip": (2 / 2) * (2 / 3)}
    q.write_text("PATH\tGROUND_TRUTH\tGREEDY\tBEAM_SEARCH\nx\tonly three\tfields\n")
    with pytest.raises(ValueError):
        M.evaluate_hypotheses(str(q))


def test_error_stats_over_two_batches_equal_one_batch_of_their_union():
    rng = np.random.default_rng(3)
    h = rng.integers(0, 4, (40, 12)).astype(np.int32)
    r = rng.integers(0, 4, (40, 9)).astype(np.int32)
    hn = rng.integers(0, 13, 40).astype(np.int32)
    rn = rng.integers(0, 10, 40).astype(np.int32)
    whole = M.ErrorStats().update(M.edit_distance_host(h, r, hn, rn))
    parts = M.ErrorStats()
    parts.update(M.edit_distance_host(h[:17], r[:17], hn[:17], rn[:17]))
    parts.update(M.edit_distance_host(h[17:], r[17:], hn[17:], rn[17:]))
    assert parts.counts() == whole.counts() and whole.pairs == 40
    assert whole.hyp_length == int(hn.sum()) and whole.ref_length == int(rn.sum())
    assert (parts.wer, parts.mer, parts.wil, parts.wip) == (whole.wer, whole.mer, whole.wil, whole.wip)


def test_zero_denominators_give_nan_and_an_empty_reference_cannot_divide_by_zero_alone():
    empty = M.ErrorStats()
    assert all(math.isnan(v) for v in (empty.wer, empty.mer, empty.wil, empty.wip, empty.error_rate))
    only_insertions = M.ErrorStats().update(M.score_texts(["uh oh"], [""], "word"))
    assert only_insertions.insertions == 2 and math.isnan(only_insertions.wer) and only_insertions.mer == 1.0
    mixed = M.ErrorStats().update(M.score_texts(["uh oh", "a"], ["", "a b"], "word"))
    assert mixed.wer == 3 / 2  # the insertions of the first pair count, its empty reference adds nothing to the denominator
    nothing_said = M.ErrorStats().update(M.score_texts([""], ["a b"], "word"))
    assert nothing_said.wer == 1.0 and nothing_said.wip == 0.0 and nothing_said.wil == 1.0


def test_pairs_wider_than_the_kernels_go_to_the_host_routine():
    W = M.EDIT_MAX_LEN + 904
    rng = np.random.default_rng(1)
    ref = rng.integers(0, 50, (2, W)).astype(np.int32)
    hyp = ref.copy()
    hyp[0, 10] = 99  # one substitution (99 is outside the alphabet)
    hyp[0, 4500:4999] = ref[0, 4501:5000]  # ref[4500] is missing from hyp[:4999]: one deletion
    out = M.edit_distance(torch.from_numpy(hyp), torch.from_numpy(ref), torch.tensor([4999, W], dtype=torch.int32),
                          torch.tensor([5000, W], dtype=torch.int32))
    assert isinstance(out, M.EditCounts) and all(isinstance(c, torch.Tensor) and c.dtype == torch.int32 for c in out)
    # pair 0: hyp[:4999] against ref[:5000] = one substitution and one deletion; pair 1 is identical over the full width
    assert table(out).tolist() == [[2, 4998, 1, 1, 0], [0, W, 0, 0, 0]]
    got = M.edit_distance(hyp, ref, np.array([4999, W]), np.array([5000, W]))  # NumPy in: the same routine
    np.testing.assert_array_equal(table(got), table(out))
