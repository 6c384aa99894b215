"""Streaming sessions of the RNN-Transducer (streaming.RnntStreamState / rnnt_encode_chunk: tfasr_lstm_infer_fwd_state, the row offsets
of tfasr_rnnt_block_tail_fwd) against the model's own offline path: after any arrival pattern a stream holds, bit for bit, the encoder
frames `model.encode` gives the utterance ALONE and the tokens `recognize` gives it, the carried LSTM states are the float64 oracle's
within the f32 bar, and a beam session holds the beam of the device search on the same frames.  `encode` is held to the reference by
tests/test_rnnt_model_gpu.py: bit-equality to it is the chain to the reference.

Tiny "ln" config of tests/rnnt_cases.py (reductions [post, post, pre] by [3, 0, 2]: two boundaries carry rows) and "noln" ([pre, pre] by
[2, 0] without LayerNorm: block 0's `pre` reduction and the two-launch tail take the gather route); three streams of 31 / 50 / 80 feature
frames, none a multiple of 6; steps of 8 feature frames (not a multiple of 6 either) and of 32; f32 and bf16."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd.schemas import PredictInput

import rnnt_cases as C
from test_rnnt_model_gpu import build

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
SAMPLES = C.SAMPLES
CHUNK = 8
F32_BAR = dict(rtol=1e-4, atol=1e-5)  # the project's single-layer bar (tests/test_ds2_gpu.py), per layer of the chain


def _prec(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


@pytest.fixture(scope="module")
def sigs():
    a = C.audio()
    return [a[b, :n].copy() for b, n in enumerate(SAMPLES)]


@pytest.fixture(scope="module")
def models(dev):
    return {(s, dt): build(dev, s, dt) for s in C.SETTINGS for dt in DT}


def _alone(m, dt, s):
    x = PredictInput(torch.from_numpy(s[None].copy()), torch.tensor([len(s)], dtype=torch.int32), m.get_initial_tokens(1), None,
                     m.get_initial_decoder_states(1))
    enc, elen = m.encode(x.inputs, x.inputs_length, precision=_prec(dt))
    m.decode_precision = _prec(dt)
    toks = m.recognize(x).tokens[0].cpu().tolist()
    return dict(enc=enc[0, :elen[0]].clone(), tokens=[t for t in toks if t != 0], n=elen[0])


@pytest.fixture(scope="module")
def alone(models, sigs):
    """per (setting, type): encoder frames and greedy tokens of every utterance run alone, computed once"""
    return {k: [_alone(m, k[1], s) for s in sigs] for k, m in models.items()}


def _session(m, dt, B=3, chunk=CHUNK, **kw):
    m.decode_precision = _prec(dt)
    rec = m.stream(B, chunk_frames=chunk, precision=_prec(dt), **kw)
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


def test_the_alone_runs_are_what_the_session_is_held_to(alone):
    for (setting, dt), rows in alone.items():
        assert [r["n"] for r in rows] == C.ELEN[setting]
        assert all(float(r["enc"].float().abs().max()) > 0.1 for r in rows) and all(len(r["tokens"]) > 3 for r in rows)
    assert all(n % 6 for n in C.FLEN)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("setting", list(C.SETTINGS))
@pytest.mark.parametrize("piece,chunk", [(1 << 20, CHUNK), (CHUNK * 160, CHUNK), (CHUNK * 160 - 1, CHUNK), (CHUNK * 160 + 1, CHUNK), (4001, 32)])
def test_arrival_patterns(models, sigs, alone, setting, dtype, piece, chunk):
    """everything at once, chunk by chunk, ragged splits one sample short of and one sample past a chunk, and the default step of 32 frames
    fed in pieces of 4001 samples; the streams finish in different steps"""
    rec = _session(models[setting, dtype], dtype, chunk=chunk)
    toks = [[] for _ in sigs]
    _feed(rec, sigs, piece, toks)
    _check(rec, toks, alone[setting, dtype])


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_both_tail_routes_stream_in_both_types(dev, sigs, dtype, route):
    """"auto" is the two launches; named, either route streams bit for bit against itself offline: the one launch places a stream's rows
    through the kernel's row offset, the two launches through a gather"""
    m = build(dev, "ln", dtype)
    m.tail_route = route
    if dtype != torch.float32:
        m.inference_twin().tail_route = route
    want = [_alone(m, dtype, s) for s in sigs]
    rec = _session(m, dtype)
    assert all(rec.enc_model._fused_tail(mod) == (route == "fused") for mod in rec.enc_model.modules)
    toks = [[] for _ in sigs]
    _feed(rec, sigs, 4001, toks)
    _check(rec, toks, want)


@pytest.mark.parametrize("dtype", DT)
def test_carried_states_are_the_oracles_and_a_slot_is_reused(models, sigs, alone, dtype):
    m = models["ln", dtype]
    ref = C.reference("ln")
    rec = _session(m, dtype)
    toks = [[], [], []]
    _feed(rec, sigs, 3000, toks)
    _check(rec, toks, alone["ln", dtype])
    st = rec.state.reference_states()
    L, P = m.cfg.nlayers, m.cfg.encoder_rnn_units
    assert st.shape == (3, L, 2, P) and st.dtype == torch.float32
    if dtype == torch.float32:  # [B, nlayers, 2, units], (h, c): the f64 oracle's states of each utterance alone, within the f32 bar per layer
        want = np.stack(ref["solo_states"])
        n = 2 * L
        np.testing.assert_allclose(st.cpu().numpy(), want, rtol=n * F32_BAR["rtol"], atol=n * F32_BAR["atol"])
    assert all(c == [0, 0, 0] for c in rec.state.cnt)  # finish left no row behind
    # a finished stream refuses samples until reset; then its slot takes another utterance from the start
    with pytest.raises(RuntimeError):
        rec.accept(torch.zeros(3, 10), [10, 0, 0])
    rec.reset(rows=[0])
    assert not rec.state.reference_states()[0].any() and rec.state.reference_states()[2].any()
    mark = len(rec.encoded_log)
    again = [[], [], []]
    x = np.zeros((3, len(sigs[2])), np.float32)
    x[0] = sigs[2]
    _take(rec.accept(torch.from_numpy(x), [len(sigs[2]), 0, 0]), again)
    _take(rec.finish(rows=[0]), again)
    assert torch.equal(_collect(rec, 0, mark), alone["ln", dtype][2]["enc"]) and again[0] == alone["ln", dtype][2]["tokens"]
    assert torch.equal(rec.state.reference_states()[0], st[2]) and torch.equal(rec.state.reference_states()[1], st[1])


@pytest.mark.parametrize("dtype", DT)
def test_encoder_state_round_trips_into_a_fresh_session(models, sigs, alone, dtype):
    m = models["ln", dtype]
    a = _session(m, dtype)
    toks = [[], [], []]
    cut = 3000  # two steps of 8 frames run: 16 rows behind block 0 = 5 groups of 3 and 1 row left; 5 rows in front of block 2 = 2 pairs and 1 left
    _take(a.accept(torch.from_numpy(np.stack([s[:cut] for s in sigs]))), toks)
    state = a.encoder_state()
    # (h, c) of three LSTMs, the carries of the two reducing boundaries (3 - 1 rows of 16, 2 - 1 rows of 48), the counts
    assert [tuple(t.shape) for t in state] == [(3, 32)] * 6 + [(3, 2, 16), (3, 1, 16), (4, 3)]
    assert state[-1].tolist() == [[0, 0, 0], [1, 1, 1], [1, 1, 1], [0, 0, 0]]
    b = _session(m, dtype)
    b.set_encoder_state(state)
    # the searches' state travels apart from the encoder's: b continues the frames, not the tokens
    rest = [s[cut:] for s in sigs]
    x = np.zeros((3, max(len(r) for r in rest)), np.float32)
    for i, r in enumerate(rest):
        x[i, :len(r)] = r
    b.buf, b.total, b.emitted = [v.copy() for v in a.buf], list(a.total), list(a.emitted)
    b.prev, b.has_prev = a.prev.copy(), a.has_prev.copy()
    b.accept(torch.from_numpy(x), [len(r) for r in rest])
    b.finish()
    for i in range(3):
        got = torch.cat([_collect(a, i), _collect(b, i)], 0)
        assert torch.equal(got, alone["ln", dtype][i]["enc"]), i
    with pytest.raises(ValueError):
        b.set_encoder_state(state[:-2] + state[-1:])


def test_a_beam_session_equals_the_device_search_on_the_same_frames(models, sigs, alone):
    dt = torch.float32
    m = models["ln", dt]
    rec = _session(m, dt, beam_width=2)
    toks = [[], [], []]
    _feed(rec, sigs, 3 * CHUNK * 160 + 7, toks)
    for b in range(3):
        assert torch.equal(_collect(rec, b), alone["ln", dt][b]["enc"])
    hyp, hlen, hscore = rec.hypotheses()
    for b in range(3):
        enc = alone["ln", dt][b]["enc"][None].contiguous()
        want, wlen, wscore, _, _ = m.recognize_beam_encoded(enc, [enc.shape[1]], 2, 2, m.get_initial_tokens(1), m.get_initial_decoder_states(1))
        k = int(wlen[0, 0])
        assert int(hlen[b, 0]) == k and torch.equal(hyp[b, 0, :k].cpu(), want[0, 0, :k].cpu()) and toks[b] == want[0, 0, :k].cpu().tolist()
        assert torch.equal(hscore[b].cpu(), wscore[0].cpu())


def test_bad_arguments(models):
    m = models["ln", torch.float32]
    with pytest.raises(ValueError):
        m.stream(1, chunk_frames=0)
    st = m.stream_state(2)
    with pytest.raises(ValueError):
        m.encode_chunk(st, torch.zeros(3, 8, 16, device=m.device), [8, 8, 8])
    with pytest.raises(ValueError):
        m.encode_chunk(st, torch.zeros(2, 8, 16, device=m.device), [9, 0])
