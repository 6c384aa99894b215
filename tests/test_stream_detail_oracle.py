"""tests/stream_detail_oracle.py (the chunked CTC greedy decoder with carried state, float64) pinned on the CPU against
recognize_detail_oracle.ctc_greedy_detail: however a [B, T, V] buffer is cut into calls - calls without frames for some rows and a last
call with nothing but the final flag included - the closed tokens in order, and the carried score, are the one-shot result exactly."""
import numpy as np
import pytest

import recognize_detail_oracle as RD
import stream_detail_oracle as SD

B, T, V = 3, 23, 5


def one_shot(logits, lens):
    ref = RD.ctc_greedy_detail(logits, lens)
    return [[(int(ref["tokens"][b, i]), int(ref["starts"][b, i]), int(ref["ends"][b, i]), ref["logp"][b, i], ref["entropy"][b, i])
             for i in range(int(ref["tokens_len"][b]))] for b in range(logits.shape[0])], ref["score"]


def random_cuts(rng, lens, zero_rate=0.3, most=6):
    """per-row frame counts per call until every row is through; a row sits a call out with probability zero_rate"""
    left, cuts = list(lens), []
    while any(left):
        take = [0 if rng.random() < zero_rate else int(min(rng.integers(1, most + 1), n)) for n in left]
        cuts.append(take)
        left = [n - t for n, t in zip(left, take)]
    return cuts


def peaked(paths, T, V, seed=0, peak=4.0):
    """logits [len(paths), T, V] whose arg-max follows each path (frames past the path: noise only)"""
    x = np.random.default_rng(seed).standard_normal((len(paths), T, V)) * 0.5
    for b, path in enumerate(paths):
        for t, c in enumerate(path):
            x[b, t, c] = peak
    return x


@pytest.mark.parametrize("seed", range(8))
def test_any_split_equals_the_one_shot_decoder(seed):
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((B, T, V)) * 2
    logits = np.repeat(logits[:, ::2], 2, 1)[:, :T] + 0.1 * rng.standard_normal((B, T, V))  # runs of two frames: tokens span boundaries
    lens = [T, int(rng.integers(0, T)), int(rng.integers(1, T + 1))]
    want, want_score = one_shot(logits, lens)
    assert sum(len(w) for w in want) >= 4 and max(e - s for w in want for _, s, e, _, _ in w) >= 2
    for k in range(6):
        cuts = random_cuts(rng, lens) if k else [lens]  # (k == 0: everything in one call)
        assert k == 0 or any(0 in c for c in cuts)
        got, state, outs = SD.run_split(logits, lens, cuts)
        assert got == want, (cuts, got, want)  # ints and float64 values, bit for bit
        assert np.array_equal(SD.score(state), want_score)
        assert all(s["open"] is None for s in state) and [s["seen"] for s in state] == lens
        # the tokens that start in each call are the plain carried decoder's: together, the one-shot tokens
        for b in range(B):
            started = [int(t) for o in outs for t in o["tokens"][b, 1:1 + int(o["tokens_len"][b])]]
            assert started == [w[0] for w in want[b]]


def test_final_flag_without_frames_closes_and_a_call_without_frames_changes_nothing():
    logits = peaked([[1, 1, 0, 2, 2]], 5, V)
    st = SD.new_state(1)
    a = SD.chunk(logits[:, :5], [5], st)
    assert a["tokens_len"][0] == 2 and a["ends"][0, :3].tolist() == [-1, 2, -1] and st[0]["open"]["cls"] == 2
    before = repr(st)
    idle = SD.chunk(np.zeros((1, 3, V)), [0], st)  # no frames, no flag: the state is untouched, the open token is reported as it stands
    assert repr(st) == before and idle["tokens_len"][0] == 0
    assert (idle["tokens"][0, 0], idle["starts"][0, 0], idle["ends"][0, 0], idle["nframes"][0, 0]) == (2, 3, -1, 2)
    assert idle["logp"][0, 0] == a["logp"][0, 2] and (idle["starts"][0, 1:] == -1).all()
    end = SD.chunk(np.zeros((1, 1, V)), [0], st, final=[1])
    assert SD.closed(end, 0) == [(2, 3, 5, a["logp"][0, 2], a["entropy"][0, 2])] and st[0]["open"] is None and st[0]["seen"] == 5


def test_hand_made_boundaries():
    #        a run over three chunks      a blank run over a boundary   c | c (one token)   c _ | c (two)      open at the end
    paths = [[0, 3, 3, 3, 3, 3, 3, 0], [1, 0, 0, 0, 0, 2, 0, 0], [0, 0, 2, 2, 2, 0, 0, 0], [0, 2, 0, 2, 0, 0, 0, 0], [0, 0, 0, 0, 0, 4, 4, 4]]
    logits = peaked(paths, 8, V, seed=3)
    lens = [8] * 5
    cuts = [[3] * 5, [2] * 5, [3] * 5]  # boundaries after frames 2 and 4
    want, want_score = one_shot(logits, lens)
    assert [[w[:3] for w in row] for row in want] == [[(3, 1, 7)], [(1, 0, 1), (2, 5, 6)], [(2, 2, 5)], [(2, 1, 2), (2, 3, 4)], [(4, 5, 8)]]
    got, state, outs = SD.run_split(logits, lens, cuts, final=False)
    assert got[:4] == want[:4] and got[4] == []  # row 4's token is still open: nothing closed yet
    assert [s["open"] is not None for s in state] == [False, False, False, False, True]
    # row 0: starts in call 0 (column 1, open), goes on through call 1 (column 0, open), closes in call 2 (column 0)
    assert (outs[0]["starts"][0, 1], outs[0]["ends"][0, 1], outs[0]["nframes"][0, 1]) == (1, -1, 2)
    assert (outs[1]["starts"][0, 0], outs[1]["ends"][0, 0], outs[1]["nframes"][0, 0], outs[1]["tokens_len"][0]) == (1, -1, 4, 0)
    assert (outs[2]["starts"][0, 0], outs[2]["ends"][0, 0], outs[2]["nframes"][0, 0]) == (1, 7, 6)
    # row 2: the same class on both sides of the boundary after frame 2 is ONE token; row 3: with a blank between, two
    assert outs[0]["tokens_len"][2] == 1 and outs[1]["tokens_len"][2] == 0 and outs[1]["tokens"][2, 0] == 2
    assert [int(o["tokens_len"][3]) for o in outs] == [1, 1, 0]
    # row 4: open at the end with the values over its three frames; the final flag then closes it at frame 8
    assert (outs[2]["starts"][4, 1], outs[2]["ends"][4, 1], outs[2]["nframes"][4, 1]) == (5, -1, 3)
    end = SD.chunk(np.zeros((5, 1, V)), [0] * 5, state, final=[1] * 5)
    assert SD.closed(end, 4) == want[4] and np.array_equal(SD.score(state), want_score)
    assert all(SD.closed(end, b) == [] for b in range(4))
