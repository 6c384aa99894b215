"""tfasr_ctc_greedy_decode_carry_detail (csrc/ctc.hip: one chunk per stream, one launch, carried state) alone, through
K.ctc_greedy_decode_carry_detail.

Held to, for every way a [B, T, V] buffer is cut into calls (chunks of 1, 2, 5 and 32 frames, a chunk longer than the kernel's 32-frame
tile, ragged rows, rows that sit calls out, the final flag with and without frames):
  - the closed tokens of all calls in order, and the carried score, are the BITS of one K.ctc_greedy_decode_detail call on the whole buffer;
  - the tokens that start in each call are the bits of K.ctc_greedy_decode_carry on the same chunk;
  - every call's output, open tokens' partial values included, against the chunked float64 decoder of tests/stream_detail_oracle.py on the
    same values (bf16: the bf16-rounded ones): integers exact, tok_logp and score (sums of n frame log-probabilities) to n atol + rtol |v|
    of the project's single-layer f32 bar (rtol 1e-4 / atol 1e-5), tok_entropy (a mean) to the bar itself;
  - unoccupied columns hold blank / -1 / -1 / 0 / 0.
The arg-max is taken on the logits themselves, which the oracle reads too, so the tokens do not depend on any margin."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

import recognize_detail_oracle as RD
import stream_detail_oracle as SD

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
T = 40
TILE = 32  # CTC_CARRY_TILE of csrc/ctc.hip
SPLITS = [1, 2, 5, 32, 37]  # frames a row gives per call at the most; 37 > TILE: the kernel's loop over frame tiles runs twice


def make_logits(seed, B, V, dtype, hold=3):
    """frames in runs of `hold` (one draw per run plus a little noise per frame) so that tokens span several frames and many chunk
    boundaries; a blank bias so that blanks separate them"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, -(-T // hold), V, generator=g) * 2
    x = base.repeat_interleave(hold, 1)[:, :T] + 0.1 * torch.randn(B, T, V, generator=g)
    x[:, :, 0] += 1.0
    return x.to(dtype)


def make_calls(seed, lens, C, sit_out=0.25):
    """[(take [B], final [B])]: every row gives min(C, what it has left) frames per call or, with probability sit_out, none; odd rows
    carry the final flag on the call that takes their last frame, and one last call has no frames and the flag for every row"""
    rng = np.random.default_rng(seed)
    left, calls = list(lens), []
    while any(left):
        take = [0 if rng.random() < sit_out else min(C, n) for n in left]
        if not any(take):
            continue
        left = [n - t for n, t in zip(left, take)]
        calls.append((take, [int(b % 2 == 1 and t > 0 and left[b] == 0) for b, t in enumerate(take)]))
    return calls + [([0] * len(lens), [1] * len(lens))]


def chunks_of(logits, calls):
    """the [B, C, V] buffer of every call (C = its longest row, at least 1; zeros past a row's frames)"""
    B, _, V = logits.shape
    pos, bufs = [0] * B, []
    for take, _ in calls:
        buf = torch.zeros(B, max(max(take), 1), V, dtype=logits.dtype)
        for b in range(B):
            buf[b, :take[b]] = logits[b, pos[b]:pos[b] + take[b]]
            pos[b] += take[b]
        bufs.append(buf)
    return bufs


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def bit(x):
    return int(np.float32(x).view(np.int32))


def run_device(dev, bufs, calls, state=None, last=None, blank=0):
    """every call through the kernel (and through the plain carried decoder, whose tokens must be the same bits) -> per-call dicts"""
    B = bufs[0].shape[0]
    state = state or K.CtcDetailState(B, dev)
    last = torch.full((B,), -1, dtype=torch.int32, device=dev) if last is None else last
    outs = []
    for buf, (take, fin) in zip(bufs, calls):
        lg, ll = buf.to(dev), torch.tensor(take, dtype=torch.int32, device=dev)
        tokens, tlen, starts, ends, logp, ent = (t.cpu().numpy() for t in K.ctc_greedy_decode_carry_detail(
            lg, ll, state, torch.tensor(fin, dtype=torch.int32, device=dev), blank=blank))
        ptok, plen = (t.cpu().numpy() for t in K.ctc_greedy_decode_carry(lg, ll, last, blank=blank))
        C = buf.shape[1]
        assert tokens.shape == (B, C + 1) and np.array_equal(tlen, plen)
        for b in range(B):
            n = int(tlen[b])
            assert np.array_equal(tokens[b, 1:n + 1], ptok[b, :n])
            free = np.arange(C + 1) > n
            free[0] = starts[b, 0] < 0
            assert (tokens[b, free] == blank).all() and (starts[b, free] == -1).all() and (ends[b, free] == -1).all()
            assert (bits(logp[b, free]) == 0).all() and (bits(ent[b, free]) == 0).all()
            occupied = np.flatnonzero(~free)
            assert (starts[b, occupied] >= 0).all() and (ends[b, occupied[:-1]] >= 0).all()  # only the last occupied column can be open
        outs.append(dict(tokens=tokens, tokens_len=tlen, starts=starts, ends=ends, logp=logp, entropy=ent))
    return outs, state


def closed_bits(outs, b):
    return [(int(o["tokens"][b, i]), int(o["starts"][b, i]), int(o["ends"][b, i]), bit(o["logp"][b, i]), bit(o["entropy"][b, i]))
            for o in outs for i in range(o["tokens"].shape[1]) if o["starts"][b, i] >= 0 and o["ends"][b, i] >= 0]


def one_shot_bits(dev, logits, lens, blank=0):
    """K.ctc_greedy_decode_detail on the whole buffer -> (per row the tokens as closed_bits gives them, score bits)"""
    tokens, tlen, starts, ends, logp, ent, score = (t.cpu().numpy() for t in K.ctc_greedy_decode_detail(
        logits.to(dev).contiguous(), torch.tensor(lens, dtype=torch.int32, device=dev), blank=blank))
    rows = [[(int(tokens[b, i]), int(starts[b, i]), int(ends[b, i]), bit(logp[b, i]), bit(ent[b, i])) for i in range(int(tlen[b]))]
            for b in range(len(lens))]
    return rows, bits(score)


def against_the_oracle(outs, bufs, calls, lens, state, blank=0):
    """every call's output against stream_detail_oracle.chunk on the same buffers -> the worst ratios to the bar"""
    B = len(lens)
    ost = SD.new_state(B)
    worst = dict(tok_logp=0.0, tok_entropy=0.0, score=0.0)
    for o, buf, (take, fin) in zip(outs, bufs, calls):
        ref = SD.chunk(buf.float().numpy(), take, ost, fin, blank)
        for k in ("tokens", "tokens_len", "starts", "ends"):
            np.testing.assert_array_equal(o[k], ref[k], err_msg=k)
        there = ref["starts"] >= 0
        assert np.isfinite(o["logp"]).all() and np.isfinite(o["entropy"]).all()
        worst["tok_logp"] = max(worst["tok_logp"], RD.ratio(o["logp"][there], ref["logp"][there], ref["nframes"][there]))
        worst["tok_entropy"] = max(worst["tok_entropy"], RD.ratio(o["entropy"][there], ref["entropy"][there]))
    nl = np.asarray(lens)
    score = state.score.cpu().numpy()
    assert state.seen.cpu().tolist() == list(lens) and not state.open.cpu().any()
    assert (bits(score[nl == 0]) == 0).all()
    worst["score"] = RD.ratio(score[nl > 0], SD.score(ost)[nl > 0], nl[nl > 0])
    assert max(worst.values()) <= 1.0, worst
    return worst


def ragged(B, seed):
    lens = np.random.default_rng(seed).integers(1, T + 1, B).tolist()
    lens[0] = T
    if B > 1:
        lens[1] = 0  # a stream that never gets a frame
    if B > 2:
        lens[2] = T - 1
    return lens


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [2, 29, 64, 65, 1000, 1027])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_any_split_gives_the_one_shot_bits(dev, B, V, dtype):
    logits = make_logits(B * 1000 + V, B, V, dtype)
    lens = ragged(B, B + V)
    want, want_score = one_shot_bits(dev, logits, lens)  # (computed once, shared by the splits)
    assert sum(len(w) for w in want) >= 3
    if V > 2:
        assert max(e - s for w in want for _, s, e, _, _ in w) >= 2  # tokens that span several frames
    for C in SPLITS:
        calls = make_calls(C + V, lens, C)
        bufs = chunks_of(logits, calls)
        if C > TILE:
            assert max(buf.shape[1] for buf in bufs) > TILE
        outs, state = run_device(dev, bufs, calls)
        for b in range(B):
            assert closed_bits(outs, b) == want[b], (C, b)
        assert np.array_equal(bits(state.score.cpu().numpy()), want_score), C
        against_the_oracle(outs, bufs, calls, lens, state)


def peaked(paths, Tn, V, seed=3, peak=4.0):
    x = torch.randn(len(paths), Tn, V, generator=torch.Generator().manual_seed(seed)) * 0.5
    for b, path in enumerate(paths):
        for t, c in enumerate(path):
            x[b, t, c] = peak
    return x


def test_hand_made_boundaries(dev):
    #        a run over three chunks      a blank run over a boundary   c | c (one token)   c _ | c (two)      open at the end
    paths = [[0, 3, 3, 3, 3, 3, 3, 0], [1, 0, 0, 0, 0, 2, 0, 0], [0, 0, 2, 2, 2, 0, 0, 0], [0, 2, 0, 2, 0, 0, 0, 0], [0, 0, 0, 0, 0, 4, 4, 4]]
    logits, lens = peaked(paths, 8, 5), [8] * 5
    calls = [([3] * 5, [0] * 5), ([2] * 5, [0] * 5), ([3] * 5, [0] * 5)]  # boundaries after frames 2 and 4
    bufs = chunks_of(logits, calls)
    want, want_score = one_shot_bits(dev, logits, lens)
    assert [[w[:3] for w in row] for row in want] == [[(3, 1, 7)], [(1, 0, 1), (2, 5, 6)], [(2, 2, 5)], [(2, 1, 2), (2, 3, 4)], [(4, 5, 8)]]
    last = torch.full((5,), -1, dtype=torch.int32, device=dev)
    outs, state = run_device(dev, bufs, calls, last=last)
    assert [closed_bits(outs, b) for b in range(4)] == want[:4] and closed_bits(outs, 4) == []
    assert state.open.cpu().tolist() == [False, False, False, False, True]
    assert (outs[0]["starts"][0, 1], outs[0]["ends"][0, 1]) == (1, -1)  # row 0: starts in call 0, goes on through call 1, closes in call 2
    assert (outs[1]["starts"][0, 0], outs[1]["ends"][0, 0], outs[1]["tokens_len"][0]) == (1, -1, 0)
    assert (outs[2]["starts"][0, 0], outs[2]["ends"][0, 0]) == (1, 7)
    assert [int(o["tokens_len"][2]) for o in outs] == [1, 0, 0] and outs[1]["tokens"][2, 0] == 2  # c | c: one token
    assert [int(o["tokens_len"][3]) for o in outs] == [1, 1, 0]  # c _ | c: two
    assert (outs[2]["starts"][4, 1], outs[2]["ends"][4, 1]) == (5, -1)
    # the partial values of the open token: the sum / the mean over its frames so far, against float64
    lsm = torch.log_softmax(logits.double(), -1)
    assert RD.ratio(outs[2]["logp"][4, 1], float(lsm[4, 5:8, 4].sum()), 3) <= 1.0
    assert RD.ratio(outs[1]["logp"][0, 0], float(lsm[0, 1:5, 3].sum()), 4) <= 1.0
    assert RD.ratio(outs[1]["entropy"][0, 0], float(RD.entropy(lsm[0, 1:5]).mean())) <= 1.0
    end_calls = [([0] * 5, [1] * 5)]
    end, state = run_device(dev, chunks_of(logits, end_calls), end_calls, state=state, last=last)
    assert closed_bits(end, 4) == want[4] and all(closed_bits(end, b) == [] for b in range(4))
    assert np.array_equal(bits(state.score.cpu().numpy()), want_score) and not state.open.cpu().any()
    against_the_oracle(outs + end, bufs + chunks_of(logits, end_calls), calls + end_calls, lens, state)


def test_a_row_reset_midway_starts_clean_while_its_neighbours_continue(dev):
    B, V = 3, 29
    first, second = make_logits(11, B, V, F32), make_logits(12, B, V, F32)
    lens = [T, T, T]
    calls = make_calls(5, lens, 5, sit_out=0.0)[:-1]  # 8 calls of 5 frames, no closing call
    bufs = chunks_of(first, calls)
    state = K.CtcDetailState(B, dev)
    last = torch.full((B,), -1, dtype=torch.int32, device=dev)
    head, _ = run_device(dev, bufs[:3], calls[:3], state, last)
    state.reset([1])  # stream 1 takes a new utterance from here on: `second`'s row 1, from its frame 0
    last[1] = -1
    assert state.ints.cpu()[1].tolist() == [-1, 0, 0, 0] and state.floats.cpu()[1].tolist() == [0.0, 0.0, 0.0]
    assert state.seen.cpu().tolist() == [15, 0, 15]
    fresh = chunks_of(second, calls)
    mixed = []
    for k in range(3, len(calls)):
        buf = bufs[k].clone()
        buf[1] = fresh[k - 3][1]
        mixed.append(buf)
    tail_calls = calls[3:] + [([0] * B, [1] * B)]
    mixed.append(torch.zeros(B, 1, V))
    tail, _ = run_device(dev, mixed, tail_calls, state, last)
    want, want_score = one_shot_bits(dev, first, lens)
    want1, want1_score = one_shot_bits(dev, second[1:2, :25].contiguous(), [25])
    assert closed_bits(head + tail, 0) == want[0] and closed_bits(head + tail, 2) == want[2]
    assert closed_bits(tail, 1) == want1[0]  # frames count from the reset
    got = bits(state.score.cpu().numpy())
    assert got[0] == want_score[0] and got[2] == want_score[2] and got[1] == want1_score[0]
    assert state.seen.cpu().tolist() == [40, 25, 40]


def test_a_call_without_frames_and_without_the_flag_leaves_the_state_untouched(dev):
    B, V = 3, 29
    logits = make_logits(31, B, V, F32)
    logits[1, 6, 0], logits[1, 7:10, 4] = 20.0, 20.0  # row 1: a blank, then a token open at the end of the first call
    state = K.CtcDetailState(B, dev)
    last = torch.full((B,), -1, dtype=torch.int32, device=dev)
    calls = [([10, 10, 10], [0, 0, 0])]
    outs, _ = run_device(dev, chunks_of(logits, calls), calls, state, last)
    assert state.open.cpu()[1] and outs[0]["ends"][1, int(outs[0]["tokens_len"][1])] == -1
    ints, floats = state.ints.clone(), state.floats.clone()
    idle_calls = [([0, 0, 5], [0, 0, 0])]  # rows 0 and 1 sit out, row 2 goes on
    idle, _ = run_device(dev, [logits[:, 10:15].contiguous()], idle_calls, state, last)
    assert torch.equal(state.ints[:2], ints[:2]) and torch.equal(state.floats[:2].view(torch.int32), floats[:2].view(torch.int32))
    assert state.seen.cpu().tolist() == [10, 10, 15]
    # the open token is reported as it stands: column 0, still open, the same partial values
    n = int(outs[0]["tokens_len"][1])
    assert idle[0]["tokens_len"][1] == 0 and (idle[0]["tokens"][1, 0], idle[0]["starts"][1, 0], idle[0]["ends"][1, 0]) == (4, 7, -1)
    assert bit(idle[0]["logp"][1, 0]) == bit(outs[0]["logp"][1, n]) and bit(idle[0]["entropy"][1, 0]) == bit(outs[0]["entropy"][1, n])
    # the flag alone (no frames) closes it at the frames seen
    end_calls = [([0, 0, 0], [0, 1, 0])]
    end, _ = run_device(dev, [torch.zeros(B, 1, V)], end_calls, state, last)
    assert (end[0]["tokens"][1, 0], end[0]["starts"][1, 0], end[0]["ends"][1, 0]) == (4, 7, 10) and not state.open.cpu()[1]
    assert bit(end[0]["logp"][1, 0]) == bit(outs[0]["logp"][1, n])
    assert torch.equal(state.ints[0], ints[0]) and state.seen.cpu().tolist() == [10, 10, 15]
