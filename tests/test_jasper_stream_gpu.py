"""Streaming JasperCTC sessions (streaming.JasperStreamState / jasper_encode_chunk, csrc/conv1d.hip) against the model's own offline
path: after any arrival pattern a stream holds, bit for bit, the encoder frames `model.encode` gives the utterance ALONE, the tokens
`recognize` gives, and in beam mode the beam the device search holds on the whole utterance's logits.

Tiny config of tests/test_jasper_gpu.py, chunk_frames 8 (4 encoder frames a step), three streams, f32 and bf16."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.schemas import PredictInput

from test_jasper_gpu import build

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
# 0.31 s, an odd number of feature frames (7361 samples -> 47 frames -> 24 encoder frames), 0.8 s
SAMPLES = [4960, 7361, 12800]
CHUNK = 8


def _prec(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


@pytest.fixture(scope="module")
def sigs():
    rng = np.random.default_rng(21)
    return [np.clip(rng.standard_normal(n) * 0.1, -1, 1).astype(np.float32) for n in SAMPLES]


@pytest.fixture(scope="module")
def models(dev):
    return {dt: build(dev, dt) for dt in DT}


@pytest.fixture(scope="module")
def alone(models, sigs):
    """per type: encoder frames, greedy tokens and f32 logits of every utterance run alone, computed once"""
    out = {}
    for dt, m in models.items():
        rows = []
        for s in sigs:
            x = PredictInput(torch.from_numpy(s[None].copy()), torch.tensor([len(s)], dtype=torch.int32))
            enc, elen = m.encode(x.inputs, x.inputs_length, precision=_prec(dt))
            m.decode_precision = _prec(dt)
            toks = m.recognize(x).tokens[0].cpu().tolist()
            logits, _ = m._infer_logits(x)
            rows.append(dict(enc=enc[0, :elen[0]].clone(), tokens=[t for t in toks if t != 0], logits=logits[:, :elen[0]].contiguous(), n=elen[0]))
        out[dt] = rows
    return out


def _session(m, dt, B=3, **kw):
    m.decode_precision = _prec(dt)
    rec = m.stream(B, chunk_frames=CHUNK, precision=_prec(dt), **kw)
    rec.encoded_log = []
    return rec


def _collect(rec, b, since=0):
    parts = [e[b, :nv[b]] for e, nv in rec.encoded_log[since:] if nv[b]]
    return torch.cat(parts, 0) if parts else None


def _feed(rec, sigs, piece, toks):
    """every stream gets `piece` samples per accept until it runs out; then finish"""
    B, pos = len(sigs), [0] * len(sigs)
    while any(pos[b] < len(sigs[b]) for b in range(B)):
        x, lens = np.zeros((B, piece), np.float32), []
        for b in range(B):
            seg = sigs[b][pos[b]:pos[b] + piece]
            x[b, :len(seg)] = seg
            lens.append(len(seg))
            pos[b] += len(seg)
        _take(rec.accept(torch.from_numpy(x), lens), toks)
    _take(rec.finish(), toks)


def _take(out, toks):
    for b in range(len(toks)):
        toks[b] += out.tokens[b, :int(out.tokens_length[b])].tolist()


def _check(rec, toks, want, rows=None, since=0):
    for b in (range(len(toks)) if rows is None else rows):
        got = _collect(rec, b, since)
        assert got is not None and got.shape == want[b]["enc"].shape and torch.equal(got, want[b]["enc"]), b
        assert toks[b] == want[b]["tokens"], b
        assert rec.frames[b] == want[b]["n"]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("piece", [1 << 20, 8 * 160, 1, 159, 160, 4001])
def test_arrival_patterns(models, sigs, alone, dtype, piece):
    """everything at once, chunk-aligned pieces (8 frames of 160 samples), and pieces of 1, 159, 160 and 4001 samples; stream 1 ends on
    an odd number of feature frames; the streams finish in different steps"""
    if piece == 1:
        sigs = [s[:2000] for s in sigs]  # 2000 accepts of one sample each (one whole step, then 5 frames at the flush)
        m = models[dtype]
        want = []
        for s in sigs:
            x = PredictInput(torch.from_numpy(s[None].copy()), torch.tensor([len(s)], dtype=torch.int32))
            enc, elen = m.encode(x.inputs, x.inputs_length, precision=_prec(dtype))
            m.decode_precision = _prec(dtype)
            want.append(dict(enc=enc[0, :elen[0]], tokens=[t for t in m.recognize(x).tokens[0].cpu().tolist() if t != 0], n=elen[0]))
    else:
        want = alone[dtype]
    rec = _session(models[dtype], dtype)
    toks = [[] for _ in sigs]
    _feed(rec, sigs, piece, toks)
    _check(rec, toks, want)
    assert sum(len(t) for t in toks) > 6


@pytest.mark.parametrize("dtype", DT)
def test_idle_stream_finish_at_different_steps_and_a_reused_slot(models, sigs, alone, dtype):
    rec = _session(models[dtype], dtype)
    toks = [[], [], []]
    step = CHUNK * 160
    first = [s[:2 * step] for s in sigs]
    _take(rec.accept(torch.from_numpy(np.stack(first))), toks)
    held = [None if t is None else t.clone() for t in rec.state.tails]
    held_cls = rec.last_class.clone()
    pos = [2 * step] * 3
    for _ in range(3):  # stream 1 is idle for three steps while the others advance
        x = np.zeros((3, step), np.float32)
        lens = [0, 0, 0]
        for b in (0, 2):
            seg = sigs[b][pos[b]:pos[b] + step]
            x[b, :len(seg)], lens[b] = seg, len(seg)
            pos[b] += len(seg)
        _take(rec.accept(torch.from_numpy(x), lens), toks)
        for t, h in zip(rec.state.tails, held):
            if t is not None:
                assert torch.equal(t[1], h[1])
        assert rec.last_class[1] == held_cls[1]
    _take(rec.finish(rows=[0]), toks)  # stream 0 ends here (its samples ran out above), the others go on
    _check(rec, toks, alone[dtype], rows=[0])
    rec.reset(rows=[0])  # ... and its slot takes utterance 2 from the start while streams 1 and 2 continue
    mark = len(rec.encoded_log)
    again = [[], [], []]
    rest = [sigs[2], sigs[1][pos[1]:], sigs[2][pos[2]:]]
    x = np.zeros((3, max(len(r) for r in rest)), np.float32)
    for b, r in enumerate(rest):
        x[b, :len(r)] = r
    _take(rec.accept(torch.from_numpy(x), [len(r) for r in rest]), again)
    _take(rec.finish(), again)
    for b in (1, 2):
        toks[b] += again[b]
    _check(rec, toks, alone[dtype], rows=[1, 2])
    got = _collect(rec, 0, mark)
    assert torch.equal(got, alone[dtype][2]["enc"]) and again[0] == alone[dtype][2]["tokens"]


@pytest.mark.parametrize("dtype", DT)
def test_encoder_state_round_trips_into_a_fresh_session(models, sigs, alone, dtype):
    m = models[dtype]
    a = _session(m, dtype)
    toks = [[], [], []]
    cut = 3 * CHUNK * 160  # two steps run; the third waits in the sample buffer for the rest of its last frame
    _take(a.accept(torch.from_numpy(np.stack([s[:cut] for s in sigs]))), toks)
    state = a.encoder_state()
    assert len(state) == sum(1 for mod in m.layers if mod["K"] > 1) and state[0].shape == (3, 10, 80)
    b = _session(m, dtype)
    b.set_encoder_state(state)
    b.last_class.copy_(a.last_class)
    b.prev[:], b.has_prev[:] = a.prev, a.has_prev
    for r in range(3):
        b.buf[r], b.total[r], b.emitted[r], b.frames[r] = a.buf[r].copy(), a.total[r], a.emitted[r], a.frames[r]
    rest = [s[cut:] for s in sigs]
    x = np.zeros((3, max(len(r) for r in rest)), np.float32)
    for r, seg in enumerate(rest):
        x[r, :len(seg)] = seg
    tail_toks = [[], [], []]
    _take(b.accept(torch.from_numpy(x), [len(r) for r in rest]), tail_toks)
    _take(b.finish(), tail_toks)
    for r in range(3):
        got = torch.cat([_collect(a, r), _collect(b, r)], 0)
        assert torch.equal(got, alone[dtype][r]["enc"]) and toks[r] + tail_toks[r] == alone[dtype][r]["tokens"], r
    with pytest.raises(ValueError):
        b.set_encoder_state(state[:-1])


@pytest.mark.parametrize("dtype", DT)
def test_beam_session_holds_the_device_searchs_beam(models, sigs, alone, dtype):
    m, W = models[dtype], 4
    rec = _session(m, dtype, beam_width=W, max_frames=64)
    toks = [[], [], []]
    B, pos, piece = 3, [0, 0, 0], 4001
    while any(pos[b] < len(sigs[b]) for b in range(B)):
        x, lens = np.zeros((B, piece), np.float32), []
        for b in range(B):
            seg = sigs[b][pos[b]:pos[b] + piece]
            x[b, :len(seg)] = seg
            lens.append(len(seg))
            pos[b] += len(seg)
        _take(rec.accept(torch.from_numpy(x), lens), toks)
        live, ln, _ = rec.hypotheses()
        for b in range(B):  # what is committed can no longer change: a prefix of the current best path
            assert toks[b] == live[b, 0, :int(ln[b, 0])].cpu().tolist()[:len(toks[b])], b
    _take(rec.finish(), toks)
    ht, hl, hs = (t.cpu() for t in rec.hypotheses())
    for b in range(B):
        wt, wl, ws = (t.cpu() for t in K.ctc_beam_search_device(alone[dtype][b]["logits"], [alone[dtype][b]["n"]], W, W, None))
        assert torch.equal(hl[b], wl[0]) and torch.equal(hs[b], ws[0]), b
        for p in range(W):
            assert ht[b, p, :int(hl[b, p])].tolist() == wt[0, p, :int(wl[0, p])].tolist(), (b, p)
        assert toks[b] == wt[0, 0, :int(wl[0, 0])].tolist(), b  # the committed outputs add up to the final best path


def test_refusals(models, dev):
    m = models[torch.float32]
    with pytest.raises(ValueError, match="multiple"):
        m.stream(1, chunk_frames=7)
    from tensorflowasr_amd import configs
    from tensorflowasr_amd.contextnet import ContextNetTransducer

    with pytest.raises(NotImplementedError):
        ContextNetTransducer(configs.contextnet_tiny(), dev, dtype=torch.float32).stream(1)
