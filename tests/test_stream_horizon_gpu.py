"""Horizon sessions (model.stream_horizon(H, ...): StreamingRecognizer with commit_horizon): a beam session runs on past max_frames by
compacting, its outputs add up to its best hypothesis, hypotheses() stays whole, and nothing depends on how the samples arrive.  The
tiny Conformer models of test_stream_beam_gpu (2 encoder frames a chunk), W = 4, max_frames = 16, commit_horizon = 8, on the 1.7 to 3 s
utterances (42 to 75 encoder frames); one Jasper session for the other stream() signatures."""
import numpy as np
import pytest
import torch

import stream_oracle as SO
from test_stream_beam_gpu import _session_inputs, rows_of
from test_stream_gpu import _tiny

pytestmark = pytest.mark.gpu
W, MAXF, H = 4, 16, 8


def _feed(rec, sigs, piece):
    """-> (tokens per stream, StreamOutput.frames of the last call); after every call the tokens so far are the start of every live
    hypothesis, after finish the best one"""
    B = len(sigs)
    toks = [[] for _ in range(B)]
    out = None

    def take(out, final):
        for b in range(B):
            toks[b] += out.tokens[b, :int(out.tokens_length[b])].tolist()
        live = rows_of(*rec.hypotheses())
        for b in range(B):
            assert rec.committed_tokens[b] == toks[b]
            if final:  # the whole best hypothesis is out
                assert toks[b] == list(live[b][0]), b
            else:
                assert all(list(y[:len(toks[b])]) == toks[b] for y in live[b]), (b, toks[b], live[b])

    n = max(len(s) for s in sigs)
    for p0 in range(0, n, piece):
        x = np.zeros((B, piece), np.float32)
        lens = []
        for b, s in enumerate(sigs):
            seg = s[p0:p0 + piece]
            x[b, :len(seg)] = seg
            lens.append(len(seg))
        take(rec.accept(torch.from_numpy(x), lens), False)
    out = rec.finish()
    take(out, True)
    return toks, out.frames.tolist()


def _session_case(model, sigs):
    B = len(sigs)
    rec = model.stream_horizon(H, B, beam_width=W, max_frames=MAXF)
    assert rec.commit_horizon == H
    toks, frames = _feed(rec, sigs, 733)
    assert all(42 <= f <= 75 for f in frames) and rec.frames == frames  # counted from the reset, far past max_frames
    assert max(rec.beam.frames) <= MAXF and any(rec.beam.dropped)  # the tries were compacted on the way, and labels left them
    base = [t.cpu() for t in rec.hypotheses(W)]
    live = rows_of(*base)
    assert sum(len(t) for t in toks) > 0 and all(len(live[b][0]) == int(base[1][b, 0]) for b in range(B))  # full sequences, full lengths
    r2 = model.stream_horizon(H, B, beam_width=W, max_frames=MAXF)
    t2, f2 = _feed(r2, sigs, 4000)
    assert t2 == toks and f2 == frames
    for a, b_ in zip(r2.hypotheses(W), base):
        assert torch.equal(a.cpu(), b_)
    # the same session without a horizon stops at max_frames, before anything of the call is taken
    plain = model.stream(B, beam_width=W, max_frames=MAXF)
    with pytest.raises(RuntimeError, match="stream 0"):
        for p0 in range(0, 24000, 4000):  # (every utterance is longer than that)
            plain.accept(torch.from_numpy(np.stack([s[p0:p0 + 4000] for s in sigs])))
    assert max(plain.frames) <= MAXF
    # compact() on demand changes no hypothesis; what reset leaves
    rec.compact()
    assert rows_of(*rec.hypotheses(W)) == live
    rec.reset(rows=[0])
    assert rec.committed_tokens[0] == [] and rec.beam.dropped[0] == [] and rows_of(*rec.hypotheses())[0] == [()]
    assert rows_of(*rec.hypotheses())[1] == live[1]
    return toks


def test_transducer_horizon_session_runs_past_max_frames(dev):
    model, sigs = _session_inputs(dev)
    _session_case(model, sigs[-3:])


def test_ctc_horizon_session_runs_past_max_frames(dev):
    model = _tiny(dev, torch.float32, head="ctc")
    _session_case(model, SO.noise(5, [1.7, 3.0, 2.2]))


def test_jasper_horizon_session_through_its_own_stream_signature(dev):
    from test_jasper_gpu import build

    m = build(dev, torch.float32)
    sig = np.clip(np.random.default_rng(21).standard_normal(12800) * 0.1, -1, 1).astype(np.float32)  # 0.8 s: 40 encoder frames
    outs = []
    for piece in (733, 4000):
        rec = m.stream_horizon(4, 1, chunk_frames=8, beam_width=W, max_frames=MAXF)  # 4 encoder frames a chunk
        toks, frames = _feed(rec, [sig], piece)
        assert frames[0] > 2 * MAXF and max(rec.beam.frames) <= MAXF
        outs.append((toks, [t.cpu() for t in rec.hypotheses(W)]))
    assert outs[0][0] == outs[1][0] and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    plain = m.stream(1, chunk_frames=8, beam_width=W, max_frames=MAXF)
    with pytest.raises(RuntimeError, match="stream 0"):
        plain.accept(torch.from_numpy(sig[None]))


def test_refusals(dev):
    model = _tiny(dev, torch.float32)
    with pytest.raises(ValueError, match="beam_width"):
        model.stream_horizon(8, 1)
    with pytest.raises(ValueError, match="beam_width"):
        model.stream_horizon(8, 1, beam_width=0)
    with pytest.raises(ValueError, match="commit_horizon"):
        model.stream_horizon(0, 1, beam_width=4)
    with pytest.raises(ValueError):
        model.stream_horizon(8, 1, beam_width=4).detailed()
    with pytest.raises(ValueError):
        model.stream_detailed(1).with_commit_horizon(8)
    rec = model.stream_horizon(8, 1, beam_width=2)
    rec.accept(torch.zeros(1, 8000))
    with pytest.raises(RuntimeError, match="before the first accept"):
        rec.with_commit_horizon(4)
