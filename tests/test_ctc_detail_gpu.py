"""tfasr_ctc_greedy_decode_detail (csrc/ctc.hip: the per-frame pass with arg-max, log-probability and entropy, and the collapse with
spans) alone, through K.ctc_greedy_decode_detail, against the NumPy float64 decoder of tests/recognize_detail_oracle.py on the same logits
(for bf16: on the bf16-rounded values).

tokens and tokens_len are bit-equal to K.ctc_greedy_decode; starts and ends are exact; tok_logp and score, sums of n frame
log-probabilities, are held to n atol + rtol |value| of the project's single-layer f32 bar (rtol 1e-4 / atol 1e-5: each term to the bar);
tok_entropy, a mean, to the bar itself.  The arg-max is taken on the logits themselves, which the oracle reads too, so the tokens do not
depend on any margin.  Each test asserts on the CPU that plain torch float32 keeps every frame under half the bar."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

import recognize_detail_oracle as RD

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
VOCABS = [2, 29, 1000, 1027]
SHAPES = [(3, 7), (5, 64)]
_PARITY = {}


def _cid(B, T, V, dtype):
    return f"B={B} T={T} V={V} {'bf16' if dtype == BF16 else 'f32'}"


ALL = [(B, T, V, dt) for (B, T) in SHAPES for V in VOCABS for dt in (F32, BF16)] + [(40, 900, 29, F32)]


@pytest.fixture(scope="module", autouse=True)
def parity_profile():
    yield
    if {_cid(*c) for c in ALL} <= set(_PARITY):  # (a partial run leaves the file alone)
        RD.write_parity("ctc_greedy_decode_detail", _PARITY)


def make_logits(seed, B, T, V, dtype, hold=3):
    """frames in runs of `hold` (one draw per run plus a little noise per frame) so that tokens span several frames; a blank bias so that
    blanks separate them"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, -(-T // hold), V, generator=g) * 2
    x = base.repeat_interleave(hold, 1)[:, :T] + 0.1 * torch.randn(B, T, V, generator=g)
    x[:, :, 0] += 1.0
    return x.to(dtype)


def f32_on_cpu_is_within_half_the_bar(logits):
    x = logits.float()
    l64, l32 = torch.log_softmax(x.double(), -1), torch.log_softmax(x, -1)
    r = (RD.ratio(l32.max(-1).values.numpy(), l64.max(-1).values.numpy()), RD.ratio(RD.entropy(l32).numpy(), RD.entropy(l64).numpy()))
    assert r[0] <= 0.5 and r[1] <= 0.5, r
    return r


def check(dev, logits, lens):
    """one call against the oracle and against K.ctc_greedy_decode -> (oracle, device results as NumPy, worst ratios)"""
    B, T, V = logits.shape
    ref = RD.ctc_greedy_detail(logits.float().numpy(), lens)
    lg = logits.to(dev).contiguous()
    ll = torch.tensor(lens, dtype=torch.int32, device=dev)
    plain_tok, plain_len = K.ctc_greedy_decode(lg, ll, blank=0)
    got = [t.cpu().numpy() for t in K.ctc_greedy_decode_detail(lg, ll, blank=0)]
    torch.cuda.synchronize()
    tokens, tlen, starts, ends, logp, ent, score = got
    assert np.array_equal(tokens, plain_tok.cpu().numpy()) and np.array_equal(tlen, plain_len.cpu().numpy())
    np.testing.assert_array_equal(tokens, ref["tokens"])
    np.testing.assert_array_equal(tlen, ref["tokens_len"])
    np.testing.assert_array_equal(starts, ref["starts"])
    np.testing.assert_array_equal(ends, ref["ends"])
    present = ref["starts"] >= 0
    assert (logp[~present] == 0).all() and (ent[~present] == 0).all()
    assert np.isfinite(logp).all() and np.isfinite(ent).all() and np.isfinite(score).all()
    nl = np.clip(np.asarray(lens), 0, T)
    r = dict(tok_logp=RD.ratio(logp[present], ref["logp"][present], ref["nframes"][present]),
             tok_entropy=RD.ratio(ent[present], ref["entropy"][present]),
             score=RD.ratio(score[nl > 0], ref["score"][nl > 0], nl[nl > 0]))
    assert (score[nl == 0] == 0).all()
    assert max(r.values()) <= 1.0, r
    return ref, got, r


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", VOCABS)
@pytest.mark.parametrize("B,T", SHAPES)
def test_against_the_oracle(dev, B, T, V, dtype):
    logits = make_logits(B * 1000 + T + V, B, T, V, dtype)
    cpu = f32_on_cpu_is_within_half_the_bar(logits)
    lens = ([0, 1, T] + [T // 2, T - 1])[:B]
    ref, _, r = check(dev, logits, lens)
    assert ref["tokens_len"][0] == 0 and ref["tokens_len"].max() >= 1
    if V > 2 and T > 7:
        assert ref["nframes"].max() >= 2  # tokens that span several frames
    _PARITY[_cid(B, T, V, dtype)] = dict(r, cpu_f32_frame_logp=cpu[0], cpu_f32_frame_entropy=cpu[1])


def test_past_the_first_pass_of_the_frame_loop(dev):
    """36000 frames: more than the 8192 workgroups x 4 waves of the per-frame launch take in one pass"""
    B, T, V = 40, 900, 29
    assert B * T > 8192 * 4
    logits = make_logits(7, B, T, V, F32)
    cpu = f32_on_cpu_is_within_half_the_bar(logits)
    g = torch.Generator().manual_seed(8)
    lens = torch.randint(0, T + 1, (B,), generator=g).tolist()
    lens[0], lens[1], lens[B - 1] = T, 0, T
    ref, _, r = check(dev, logits, lens)
    assert ref["tokens_len"].max() > 100
    _PARITY[_cid(B, T, V, F32)] = dict(r, cpu_f32_frame_logp=cpu[0], cpu_f32_frame_entropy=cpu[1])


def test_hand_built_paths(dev):
    V, T, PEAK = 5, 10, 4.0
    #        c c _ c         c d     run to the last valid frame   run into the padding    all blank   a tie of classes 2 and 4
    paths = [[2, 2, 0, 2], [2, 3], [0, 1, 1, 1], [3, 3, 3, 3, 3, 3], [0] * T, [(2, 4), (2, 4), 0]]
    lens = [4, 2, 4, 3, T, 3]
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(len(paths), T, V, generator=g) * 0.5
    for b, path in enumerate(paths):
        for t, c in enumerate(path):
            logits[b, t, list(c) if isinstance(c, tuple) else c] = PEAK
    assert logits[5, 0, 2] == logits[5, 0, 4] == logits[5, 0].max()
    f32_on_cpu_is_within_half_the_bar(logits)
    ref, (tokens, tlen, starts, ends, logp, ent, score), _ = check(dev, logits, lens)
    assert tlen.tolist() == [2, 2, 1, 1, 0, 1]
    assert tokens[0, :2].tolist() == [2, 2] and (starts[0, :2].tolist(), ends[0, :2].tolist()) == ([0, 3], [2, 4])
    assert tokens[1, :2].tolist() == [2, 3] and (starts[1, :2].tolist(), ends[1, :2].tolist()) == ([0, 1], [1, 2])
    assert tokens[2, 0] == 1 and (starts[2, 0], ends[2, 0]) == (1, 4)
    assert tokens[3, 0] == 3 and (starts[3, 0], ends[3, 0]) == (0, 3)  # the frames past logit_len do not count ...
    lsm = torch.log_softmax(logits.double(), -1)
    assert RD.ratio(logp[3, 0], float(lsm[3, :3, 3].sum()), 3) <= 1.0  # ... nor do their log-probabilities
    assert (starts[4] == -1).all() and (ends[4] == -1).all() and RD.ratio(score[4], float(lsm[4, :, 0].sum()), T) <= 1.0
    assert tokens[5, 0] == 2 and (starts[5, 0], ends[5, 0]) == (0, 2)  # the first of two equal maxima
    assert RD.ratio(logp[5, 0], float(lsm[5, :2, 2].sum()), 2) <= 1.0
