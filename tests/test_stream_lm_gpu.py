"""Streaming sessions with an n-gram LM fused into the carried beam (model.stream_lm(lm, ..., beam_width >= 1), K.CtcLmBeamStream): a
Jasper stream ends on the n-best list recognize_nbest_lm gives the utterance alone, a Conformer CTC stream on the fused one-shot search
over the session's own encoder frames, however the samples arrive; a horizon session runs past max_frames; every refusal; and lm=None
changes nothing.  The tiny models and helpers of test_stream_beam_gpu / test_jasper_stream_gpu / test_stream_horizon_gpu, W = 4."""
import numpy as np
import pytest
import torch

import stream_oracle as SO
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.lm import NGramLM
from tensorflowasr_amd.schemas import PredictInput
from test_jasper_gpu import build
from test_jasper_stream_gpu import _feed as jasper_feed
from test_jasper_stream_gpu import _collect, _session, sigs  # noqa: F401  (sigs: the module's fixture)
from test_stream_beam_gpu import _feed_beam, _logged, _session_inputs, rows_of
from test_stream_gpu import _tiny
from test_stream_horizon_gpu import _feed as horizon_feed

pytestmark = pytest.mark.gpu
W = 4
ALPHA, BETA = 0.8, 0.3
NAMES = ("tokens", "lengths", "score", "log_prob", "lm_score")


def small_lm(V, blank, order=3):
    """estimated from a dozen token sequences with a few favourite successors"""
    rng = np.random.default_rng(V)
    toks = [t for t in range(V) if t != blank]
    seqs = []
    for _ in range(12):
        s = [toks[int(rng.integers(len(toks)))]]
        for _ in range(int(rng.integers(2, 9))):
            s.append(toks[(toks.index(s[-1]) * 3 + int(rng.integers(2))) % len(toks)])
        seqs.append(s)
    return NGramLM.estimate(seqs, order, V, blank)


@pytest.fixture(scope="module")
def jasper(dev):
    return build(dev, torch.float32)


def test_jasper_stream_ends_on_the_offline_fused_nbest(jasper, sigs):  # noqa: F811
    m = jasper
    lm = small_lm(m.cfg.vocab_size, m.blank)
    alone = []
    for s in sigs:
        x = PredictInput(torch.from_numpy(s[None].copy()), torch.tensor([len(s)], dtype=torch.int32))
        enc, elen = m.encode(x.inputs, x.inputs_length, precision="f32")
        nbest = [t.cpu() for t in m.recognize_nbest_lm(x, lm, beam_width=W, top_paths=W, alpha=ALPHA, beta=BETA)]
        top = m.recognize_beam_lm(x, lm, beam_width=W, alpha=ALPHA, beta=BETA).tokens[0].cpu().tolist()
        alone.append(dict(enc=enc[0, :elen[0]].clone(), nbest=nbest, top=top, n=int(elen[0])))
    outs = []
    for piece in (733, 4000):
        rec = _session(m, torch.float32, beam_width=W, max_frames=64).with_lm(lm, ALPHA, BETA)
        assert isinstance(rec.beam, K.CtcLmBeamStream) and rec.beam.blank_index == m.blank
        toks = [[] for _ in sigs]
        jasper_feed(rec, sigs, piece, toks)
        have = [t.cpu() for t in rec.hypotheses_lm(W)]
        three = [t.cpu() for t in rec.hypotheses(W)]
        assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, have[:3]))  # the three-tuple, scores = score
        for b, want in enumerate(alone):
            got = _collect(rec, b)
            assert got.shape == want["enc"].shape and torch.equal(got, want["enc"]), b  # the offline frames, bit for bit
            wt, wl, ws, wlp, wls = want["nbest"]
            assert torch.equal(have[1][b], wl[0]), (piece, b)
            for p in range(W):
                assert have[0][b, p, :int(wl[0, p])].tolist() == wt[0, p, :int(wl[0, p])].tolist(), (piece, b, p)
                assert not have[0][b, p, int(wl[0, p]):].any()
            np.testing.assert_array_equal(have[4][b].numpy().view(np.int32), wls[0].numpy().view(np.int32))  # lm_score, exactly
            np.testing.assert_allclose(have[3][b].numpy(), wlp[0].numpy(), rtol=0, atol=1e-4)
            assert torch.equal(have[2][b], have[3][b] + have[4][b])
            n = int(wl[0, 0])
            assert toks[b] == want["top"][:n] and not any(want["top"][n:]), (piece, b)  # the emitted tokens add up to recognize_beam_lm's
        outs.append((toks, have))
    assert outs[0][0] == outs[1][0] and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert sum(len(t) for t in outs[0][0]) > 0


def test_conformer_ctc_stream_holds_the_fused_search_on_its_own_frames(dev):
    model = _tiny(dev, torch.float32, head="ctc")
    lm = small_lm(model.cfg.vocab_size, model.blank)
    sigs_ = SO.noise(5, [1.7, 3.0, 2.2])
    B = len(sigs_)
    rec = model.stream_lm(lm, B, beam_width=W, lm_alpha=ALPHA, lm_beta=BETA)
    toks, trace = _feed_beam(rec, sigs_, 733)  # (committed tokens are a prefix of the best hypothesis after every call, all of it at the end)
    enc, lens = _logged(rec, B)
    logits = K.matmul(enc.float().reshape(-1, enc.shape[2]).contiguous(), model.ps.p2d("dec/logits/w"), bias=model.ps.p("dec/logits/b"))
    logits = logits.view(B, enc.shape[1], -1)
    want = K.ctc_beam_search_lm(logits, lens, lm.tables(ALPHA, BETA), beam_width=W, top_paths=W, blank_index=model.blank)
    have = rec.hypotheses_lm(W)
    for name, a, b in zip(NAMES, have, want):
        assert torch.equal(a.cpu(), b.cpu()), name
    live = rows_of(*have[:3])
    assert [list(live[b][0]) for b in range(B)] == toks and sum(len(t) for t in toks) > 0
    r2 = model.stream_lm(lm, B, beam_width=W, lm_alpha=ALPHA, lm_beta=BETA)
    t2, _ = _feed_beam(r2, sigs_, 4000)
    assert t2 == toks
    for a, b in zip(r2.hypotheses_lm(W), have):
        assert torch.equal(a.cpu(), b.cpu())
    # a stream that is still running ranks without the end-of-sentence term, a finished one with it
    r3 = model.stream_lm(lm, B, beam_width=W, lm_alpha=ALPHA, lm_beta=BETA)
    n = min(len(s) for s in sigs_)
    r3.accept(torch.from_numpy(np.stack([s[:n] for s in sigs_])))
    run = [t.cpu() for t in r3.hypotheses_lm(W)]
    r3.finish(rows=[0])  # stream 0 ended with these samples
    fin = [t.cpu() for t in r3.hypotheses_lm(W)]
    tables = lm.tables(ALPHA, BETA)
    for b in (1, 2):
        for a, b_ in zip(run, fin):
            assert torch.equal(a[b, :, :run[0].shape[2]] if a.dim() == 3 else a[b], b_[b, :, :run[0].shape[2]] if a.dim() == 3 else b_[b])
    for t, with_term in ((run, False), (fin, True)):
        for p in range(W):
            if float(t[3][0, p]) == -np.inf:
                continue
            st, acc = tables.start, np.float32(0.0)
            for c in t[0][0, p, :int(t[1][0, p])].tolist():
                inc, st = NGramLM.walk(tables, st, int(c))
                acc = np.float32(acc + inc)
            if with_term and tables.eos >= 0:
                acc = np.float32(acc + NGramLM.walk(tables, st, tables.eos, eos=True)[0])
            assert float(t[4][0, p]) == float(acc), (with_term, p)
    assert tables.eos >= 0


def test_horizon_session_with_an_lm_runs_past_max_frames(dev):
    model = _tiny(dev, torch.float32, head="ctc")
    lm = small_lm(model.cfg.vocab_size, model.blank)
    sigs_ = SO.noise(5, [1.7, 3.0, 2.2])
    B, MAXF = len(sigs_), 16
    outs = []
    for piece in (733, 4000):
        rec = model.stream_horizon(8, B, beam_width=W, max_frames=MAXF, lm=lm, lm_alpha=ALPHA, lm_beta=BETA)
        assert rec.commit_horizon == 8 and isinstance(rec.beam, K.CtcLmBeamStream)
        toks, frames = horizon_feed(rec, sigs_, piece)  # (the outputs add up to the best hypothesis: asserted there)
        assert all(f > 2 * MAXF for f in frames) and max(rec.beam.frames) <= MAXF and any(rec.beam.dropped)
        have = [t.cpu() for t in rec.hypotheses_lm(W)]
        three = [t.cpu() for t in rec.hypotheses(W)]
        assert all(torch.equal(a, b) for a, b in zip(three, have[:3]))
        live = rows_of(*three)
        for b in range(B):  # full sequences, full lengths, the committed part included
            assert len(live[b][0]) == int(have[1][b, 0]) >= len(rec.beam.dropped[b]) and list(live[b][0]) == toks[b]
            assert all(list(y[:len(rec.beam.dropped[b])]) == rec.beam.dropped[b] for y in live[b])
        assert torch.equal(have[2], have[3] + have[4])
        outs.append((toks, have))
    assert outs[0][0] == outs[1][0] and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))
    assert sum(len(t) for t in outs[0][0]) > 0


def test_refusals(dev, jasper):
    model = _tiny(dev, torch.float32, head="ctc")
    lm = small_lm(model.cfg.vocab_size, model.blank)
    with pytest.raises(ValueError, match="beam_width >= 1"):
        model.stream_lm(lm, 1)
    with pytest.raises(ValueError, match="beam_width >= 1"):
        model.stream(1).with_lm(lm)
    with pytest.raises(ValueError, match="32"):
        model.stream_lm(lm, 1, beam_width=33)
    with pytest.raises(ValueError, match="detail"):
        model.stream_detailed(1).with_lm(lm)
    with pytest.raises(ValueError, match="detail"):
        model.stream_lm(lm, 1, beam_width=4).detailed()
    with pytest.raises(ValueError, match="language model"):
        model.stream_lm(small_lm(model.cfg.vocab_size - 1, model.blank), 1, beam_width=4)
    with pytest.raises(ValueError, match="beam_width >= 1"):
        jasper.stream_lm(small_lm(jasper.cfg.vocab_size, jasper.blank), 1, chunk_frames=8)
    with pytest.raises(ValueError, match="hypotheses_lm"):
        model.stream(1, beam_width=4).hypotheses_lm()
    rec = model.stream(1, beam_width=4)
    rec.accept(torch.zeros(1, 8000))
    with pytest.raises(RuntimeError, match="before the first accept"):
        rec.with_lm(lm)
    transducer, _ = _session_inputs(dev)
    with pytest.raises(NotImplementedError, match="prediction network is its LM"):
        transducer.stream_lm(lm, 1, beam_width=4)
    with pytest.raises(NotImplementedError, match="prediction network is its LM"):
        transducer.stream(1, beam_width=4).with_lm(lm)


def test_lm_none_changes_nothing(dev):
    model = _tiny(dev, torch.float32, head="ctc")
    sigs_ = SO.noise(5, [1.7, 3.0, 2.2])
    B = len(sigs_)
    a = model.stream(B, beam_width=W)
    b = model.stream_lm(None, B, beam_width=W, lm_alpha=0.9, lm_beta=0.4)
    assert type(a.beam) is type(b.beam) is K.CtcBeamStream and b.beam.blank_index == model.cfg.vocab_size - 1
    ta, _ = _feed_beam(a, sigs_, 733)
    tb, _ = _feed_beam(b, sigs_, 733)
    assert ta == tb and sum(len(t) for t in ta) > 0
    for x, y in zip(a.hypotheses(W), b.hypotheses(W)):
        assert torch.equal(x, y)
    g = model.stream_lm(None, B)  # the greedy session too
    assert g.beam is None and model.stream_horizon(8, B, beam_width=W, lm=None).lm_tables is None
