"""Streaming sessions of the unidirectional DeepSpeech2 (streaming.DS2StreamState / ds2_encode_chunk: tfasr_lstm_infer_fwd_state,
tfasr_stream_rowconv_fwd, conv2d_fwd(lead)) against the model's own offline path: after any arrival pattern a stream holds, bit for bit,
the encoder frames `model.encode` gives the utterance ALONE, the tokens `recognize` gives, and in beam mode the beam the device search
holds on the whole utterance's logits.  `encode` of these utterances is held to the float64 oracle by tests/test_ds2_gpu.py: bit-equality
to it is the chain to the reference.

Tiny `uni` config of tests/ds2_cases.py (seed 12), chunk_frames 8 (4 encoder frames a step), three streams, f32 and bf16."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC
from tensorflowasr_amd.schemas import PredictInput, TrainData, TrainInput, TrainLabel

import ds2_cases as C
from test_ds2_gpu import build

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
# 0.31 s, an odd number of feature frames (7361 samples -> 47 frames -> 24 encoder frames), 0.8 s
SAMPLES = [4960, 7361, 12800]
CHUNK = 8


def _prec(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


@pytest.fixture(scope="module")
def sigs():
    rng = np.random.default_rng(5)
    return [np.clip(rng.standard_normal(n) * 0.1, -1, 1).astype(np.float32) for n in SAMPLES]


@pytest.fixture(scope="module")
def models(dev):
    return {dt: build(dev, "uni", dt) for dt in DT}


def _alone(m, dt, s, logits=False):
    x = PredictInput(torch.from_numpy(s[None].copy()), torch.tensor([len(s)], dtype=torch.int32))
    enc, elen = m.encode(x.inputs, x.inputs_length, precision=_prec(dt))
    m.decode_precision = _prec(dt)
    toks = m.recognize(x).tokens[0].cpu().tolist()
    row = dict(enc=enc[0, :elen[0]].clone(), tokens=[t for t in toks if t != 0], n=elen[0])
    if logits:
        row["logits"] = m._infer_logits(x)[0][:, :elen[0]].contiguous()
    return row


@pytest.fixture(scope="module")
def alone(models, sigs):
    """per type: encoder frames, greedy tokens and f32 logits of every utterance run alone, computed once"""
    return {dt: [_alone(m, dt, s, logits=True) for s in sigs] for dt, m in models.items()}


def _session(m, dt, B=3, **kw):
    m.decode_precision = _prec(dt)
    rec = m.stream(B, chunk_frames=CHUNK, precision=_prec(dt), **kw)
    rec.encoded_log = []
    return rec


def _collect(rec, b, since=0):
    parts = [e[b, :nv[b]] for e, nv in rec.encoded_log[since:] if nv[b]]
    return torch.cat(parts, 0) if parts else None


def _take(out, toks):
    for b in range(len(toks)):
        toks[b] += out.tokens[b, :int(out.tokens_length[b])].tolist()


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


def _check(rec, toks, want, rows=None, since=0):
    for b in (range(len(toks)) if rows is None else rows):
        got = _collect(rec, b, since)
        assert got is not None and got.shape == want[b]["enc"].shape and torch.equal(got, want[b]["enc"]), b
        assert toks[b] == want[b]["tokens"], b
        assert rec.frames[b] == want[b]["n"]


def test_the_alone_runs_are_what_the_session_is_held_to(models, alone):
    """the frame counts (31, 47 and 80 feature frames over the time stride 2) and a comparison that is not empty"""
    for dt in DT:
        assert [r["n"] for r in alone[dt]] == [16, 24, 40]
        assert all(float(r["enc"].float().abs().max()) > 0.1 for r in alone[dt])
        assert sum(len(r["tokens"]) for r in alone[dt]) > 6


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("piece", [1 << 20, 8 * 160, 1, 159, 160, 4001])
def test_arrival_patterns(models, sigs, alone, dtype, piece):
    """everything at once, chunk-aligned pieces (8 frames of 160 samples), and pieces of 1, 159, 160 and 4001 samples; stream 1 ends on
    an odd number of feature frames; the streams finish in different steps"""
    if piece == 1:
        sigs = [s[:2000] for s in sigs]  # 2000 accepts of one sample each (one whole step, then 5 frames at the flush)
        want = [_alone(models[dtype], dtype, s) for s in sigs]
    else:
        want = alone[dtype]
    rec = _session(models[dtype], dtype)
    toks = [[] for _ in sigs]
    _feed(rec, sigs, piece, toks)
    _check(rec, toks, want)
    assert sum(len(t) for t in toks) > (2 if piece == 1 else 6)


def _offline_states(m, dt, s):
    """[nlayers, 2, P]: (h_last, c_last) of every LSTM in the offline run of one utterance alone (DeepSpeech2CTC.encoder_fwd's calls)"""
    em = m.inference_twin() if dt == torch.float32 else m
    dev = em.device
    feats, flen = em.frontend(torch.from_numpy(s[None].copy()).to(dev), [len(s)])
    x = em.conv_module_fwd(feats)
    T = x.shape[1]
    lens = em._h2d([em.cfg.encoder_length(flen[0])])
    x = x.view(1, T, -1)
    out = []
    for r in em.modules["rnns"]:
        k, b, rk = em._rnn_consts(r)
        xg = K.matmul(x.view(T, x.shape[2]), k, bias=b).view(1, T, k.shape[1])
        y, h, c = K.lstm_infer_fwd(xg, rk, lens, ndir=1, want_state=True)
        out.append(torch.stack([h[0, 0], c[0, 0]]))
        scale, shift = em._affine(r["rowconv"] + "/bn")
        x = K.channel_affine_fwd(K.dwconv_fwd(y, em.ps.p(r["rowconv"] + "/conv/w"), None), scale, shift, relu=True)
    return torch.stack(out)


@pytest.mark.parametrize("dtype", DT)
def test_idle_stream_finish_at_different_steps_and_a_reused_slot(models, sigs, alone, dtype):
    m = models[dtype]
    rec = _session(m, dtype)
    toks = [[], [], []]
    step = CHUNK * 160
    first = [s[:2 * step] for s in sigs]
    _take(rec.accept(torch.from_numpy(np.stack(first))), toks)
    held = [t.clone() for t in rec.state.export()]
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
        for t, h in zip(rec.state.export(), held):
            assert torch.equal(t[1], h[1]) and not torch.equal(t[2], h[2])
        assert rec.last_class[1] == held_cls[1]
    _take(rec.finish(rows=[0]), toks)  # stream 0 ends here (its samples ran out above), the others go on
    _check(rec, toks, alone[dtype], rows=[0])
    # the LSTM states of the finished stream, in the reference's layout, are those of the offline run of that utterance alone
    ref = rec.state.reference_states()
    nl, P = len(m.modules["rnns"]), m.cfg.rnn_units
    assert ref.shape == (3, nl, 2, P) and ref.dtype == torch.float32
    assert torch.equal(ref[0], _offline_states(m, dtype, sigs[0]))
    rec.reset(rows=[0])  # ... and its slot takes utterance 2 from the start while streams 1 and 2 continue
    assert not rec.state.reference_states()[0].any() and rec.state.reference_states()[2].any()
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
    want = torch.stack([_offline_states(m, dtype, sigs[b]) for b in (2, 1, 2)])
    assert torch.equal(rec.state.reference_states(), want)


@pytest.mark.parametrize("dtype", DT)
def test_encoder_state_round_trips_into_a_fresh_session(models, sigs, alone, dtype):
    m = models[dtype]
    a = _session(m, dtype)
    toks = [[], [], []]
    cut = 3 * CHUNK * 160  # two steps run; the third waits in the sample buffer for the rest of its last frame
    _take(a.accept(torch.from_numpy(np.stack([s[:cut] for s in sigs]))), toks)
    state = a.encoder_state()
    # two conv tails, (h, c) of two LSTMs, two RowConv1D tails (K = 5)
    assert [tuple(t.shape) for t in state] == [(3, 4, 16), (3, 2, 8 * 16), (3, 32), (3, 32), (3, 32), (3, 32), (3, 4, 32), (3, 4, 32)]
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


@pytest.mark.parametrize("B,dtype", [(17, torch.float32), (17, torch.bfloat16), (65, torch.bfloat16)])
def test_batch_tiles_and_persistent_slices(models, sigs, B, dtype):
    """B = 17: two batch tiles of the recurrence; B = 65 in bf16: two slices of the persistent launch (64 streams + 1).  The short audio
    cut to five lengths, everything at once: every row is the utterance alone."""
    m = models[dtype]
    cuts = [sigs[0][:len(sigs[0]) - 163 * k] for k in range(5)]
    want = [_alone(m, dtype, s) for s in cuts]
    rec = _session(m, dtype, B=B)
    x = np.zeros((B, len(sigs[0])), np.float32)
    for b in range(B):
        x[b, :len(cuts[b % 5])] = cuts[b % 5]
    toks = [[] for _ in range(B)]
    _take(rec.accept(torch.from_numpy(x), [len(cuts[b % 5]) for b in range(B)]), toks)
    _take(rec.finish(), toks)
    _check(rec, toks, [want[b % 5] for b in range(B)])


def test_refusals(models, dev):
    uni = models[torch.float32]
    with pytest.raises(ValueError, match="multiple"):
        uni.stream(1, chunk_frames=7)
    with pytest.raises(ValueError, match="multiple"):
        uni.stream(1, chunk_frames=0)
    bi = build(dev, "bi")
    same = DeepSpeech2CTC(C.tiny_config("uni", conv_padding="same"), dev, dtype=torch.float32, seed=1)
    for model, why in ((bi, "rnn_bidirectional"), (same, "conv_padding")):
        for call in (lambda: model.stream(), lambda: model.stream(batch_size=-5, chunk_frames=7), lambda: model.stream_state(),
                     lambda: model.encode_chunk(None, None, None)):
            with pytest.raises(NotImplementedError, match="inference only.*cannot be streamed.*" + why):
                call()
    data = TrainData(TrainInput(torch.zeros(1, 1600), torch.tensor([1600]), None, None), TrainLabel(torch.ones(1, 2, dtype=torch.int32), torch.tensor([2])))
    for call in (lambda: uni.train_step(data), lambda: uni.loss_and_backward(data), lambda: uni.compile()):
        with pytest.raises(NotImplementedError, match="inference only"):
            call()
