"""Commit horizon and trie compaction of the beam streams (K.RnntBeamStream / K.CtcBeamStream: commit(horizon=H), compact()):
compaction changes nothing a caller can see; a horizon that never fires changes nothing; the rule against the float64 oracle
(tests/beam_horizon_oracle.py); a stream that compacts runs past its capacity bit-equal to one with room for everything; reset."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

import beam_horizon_oracle as HO
from test_rnnt_beam_gpu import LENS, SEARCH_CASES, Net, sharpened, signals
from test_stream_beam_gpu import C_LENS, T_LENS, chunk_of, model_weights, plan, rand_weights, rows_of

pytestmark = pytest.mark.gpu
NEG = -np.inf


# ------------------------------------------------------------------------------------------------------------------ helpers
def full_beam(stream, W):
    """-> (per stream the live rows' FULL label tuples (dropped labels + what the trie holds), best first; the other n-best tensors)"""
    out = [t.cpu() for t in stream.nbest(W)]
    toks, lens, scores = out[:3]
    rows = [[tuple(stream.dropped[b]) + tuple(toks[b, p, :int(lens[b, p])].tolist()) for p in range(W) if float(scores[b, p]) != NEG]
            for b in range(stream.B)]
    for b in range(stream.B):  # dead rows are empty, padding is the pad value
        pad = stream.blank if hasattr(stream, "blank") else 0
        for p in range(W):
            n = int(lens[b, p])
            assert (toks[b, p, n:] == pad).all() and (n == 0 or float(scores[b, p]) != NEG)
    return rows, out[2:]


def assert_same_beam(a, b, W, what):
    ra, ta = full_beam(a, W)
    rb, tb = full_beam(b, W)
    assert ra == rb, (what, ra, rb)
    for x, y in zip(ta, tb):  # scores, and for the transducer next_tok / next_h / next_c
        assert torch.equal(x, y), what


def take(stream, got, **kw):
    toks, n = stream.commit(**kw)
    toks, n = toks.cpu(), n.cpu()
    for b in range(len(got)):
        got[b] += toks[b, :int(n[b])].tolist()


def kept_nodes(rows, dropped):
    """the trie a compaction leaves: the root and one node per distinct non-empty prefix of the live rows below it"""
    return 1 + len({y[len(dropped):k] for y in rows for k in range(len(dropped) + 1, len(y) + 1)})


def neutral(make, x, lens, C, W, what):
    """a stream that commits and compacts after every step against a twin that does neither"""
    s, twin = make(), make()
    got = [[] for _ in lens]
    for start, nv in plan(lens, C):
        xc = chunk_of(x, start, nv, C)
        s.advance(xc, nv)
        twin.advance(xc, nv)
        take(s, got)
        res = s.compact()
        assert_same_beam(s, twin, W, (what, start))
        rows, _ = full_beam(s, W)
        for b, (drop, nodes, frames) in enumerate(res):
            d = s.dropped[b]
            assert got[b][:len(d)] == d and len(d) <= len(got[b])  # what left the trie had been committed
            assert nodes == kept_nodes(rows[b], d), (what, b)
            assert frames == s.frames[b] == max(len(y) for y in rows[b]) - len(d)
    return sum(len(d) for d in s.dropped)


# ------------------------------------------------------------------------------------------------------------------ 3: compaction is neutral
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [6, 29])
def test_ctc_compaction_is_neutral(dev, V, dtype):
    B, T = 3, 19
    rng = np.random.default_rng(V)
    dropped = 0
    for W in (1, 2, 8, 64):
        for blank in (0, V - 1):
            x = torch.from_numpy((rng.standard_normal((B, T, V)) * 2.0).astype(np.float32)).to(dev).to(dtype)
            for C in (1, 4):
                dropped += neutral(lambda: K.CtcBeamStream(B, C, T, V, W, blank_index=blank, device=dev), x, C_LENS, C, W, (V, W, blank, C))
    assert dropped > 0, "input condition: some compaction drops labels"


@pytest.mark.parametrize("V", [3, 29, 1000])
def test_transducer_compaction_is_neutral(dev, V):
    B, T, Tcap, E, U, J = 4, 23, 64, 24, 24, 40
    w = rand_weights(dev, V, E, U, J, seed=V + U)
    encj = torch.randn(B, T, J, generator=torch.Generator().manual_seed(7)).to(dev)
    dropped = 0
    for W in (1, 2, 10, 64):
        for C in (1, 5):
            dropped += neutral(lambda: K.RnntBeamStream(w, B, Tcap, W, blank=0), encj, T_LENS, C, W, (V, W, C))
    assert dropped > 0, "input condition: some compaction drops labels"


def test_transducer_compaction_is_neutral_with_packed_weights(dev):
    B, T, Tcap, V, E, U, J, W = 4, 23, 64, 29, 32, 32, 48, 10
    w = rand_weights(dev, V, E, U, J, seed=V + U)
    pk = K.decode_pack(w[0], w[1], w[2], w[6], w[8])
    assert pk is not None
    encj = torch.randn(B, T, J, generator=torch.Generator().manual_seed(7)).to(dev)
    neutral(lambda: K.RnntBeamStream(w, B, Tcap, W, blank=0, packed=pk), encj, T_LENS, 5, W, "packed")


def test_ctc_compaction_at_a_prefix_reentry(dev):
    """the logits and the cuts of test_stream_beam_gpu.test_ctc_prefix_reentry_across_a_chunk_boundary, a commit and a compaction at the
    cut: a prefix that is out of the beam there has lost its node, and comes back on a fresh one with the same mass"""
    x = torch.from_numpy((np.random.default_rng(5).standard_normal((300, 14, 3)) * 1.5).astype(np.float32)).to(dev)
    B, T, V, W = 300, 14, 3, 2
    want = [t.cpu() for t in K.ctc_beam_search_device(x, [T] * B, W, W, 0)]
    s = K.CtcBeamStream(B, 1, T, V, W, blank_index=0, device=dev)
    beams = []
    for t in range(T):
        s.advance(x[:, t:t + 1].contiguous(), [1] * B)
        beams.append([set(r) for r in rows_of(*s.nbest(W))])
    cuts = set()
    for b in range(B):
        for t in range(2, T):
            back = [y for y in beams[t][b] if y in beams[t - 2][b] and y not in beams[t - 1][b]]
            if any(any(len(e) > len(y) and e[:len(y)] == y for e in beams[t - 1][b]) for y in back):
                cuts.add(t)
    assert cuts, "input condition: a prefix leaves the beam and re-enters while an extension of it stayed"
    for cut in sorted(cuts)[:3]:
        s = K.CtcBeamStream(B, T, T, V, W, blank_index=0, device=dev)
        s.advance(x[:, :cut].contiguous(), [cut] * B)
        s.commit()
        s.compact()
        s.advance(x[:, cut:].contiguous(), [T - cut] * B)
        rows, (scores,) = full_beam(s, W)
        assert torch.equal(scores, want[2]), cut
        assert rows == rows_of(*want), cut
    assert any(s.dropped)


# ------------------------------------------------------------------------------------------------------------------ 4: a horizon that never fires
def _never_fires(make, x, lens, C, W, H):
    a, b = make(), make()
    ga, gb = [[] for _ in lens], [[] for _ in lens]
    for start, nv in plan(lens, C):
        xc = chunk_of(x, start, nv, C)
        a.advance(xc, nv)
        b.advance(xc, nv)
        take(a, ga, horizon=H)
        take(b, gb)
        assert ga == gb
        assert_same_beam(a, b, W, start)
    take(a, ga, final_rows=range(len(lens)), horizon=H)
    take(b, gb, final_rows=range(len(lens)))
    assert ga == gb and sum(len(g) for g in ga) > 0
    assert a.hstate[:, 0].tolist() == list(lens)  # the state's frame counts


def test_a_horizon_that_never_fires_changes_nothing(dev):
    B, T, V = 3, 19, 6
    x = torch.from_numpy((np.random.default_rng(1).standard_normal((B, T, V)) * 2.0).astype(np.float32)).to(dev)
    for W in (2, 8):
        for C in (1, 4):
            _never_fires(lambda: K.CtcBeamStream(B, C, T, V, W, device=dev), x, C_LENS, C, W, T)
    w = rand_weights(dev, 29, 24, 24, 40, seed=53)
    encj = torch.randn(4, 23, 40, generator=torch.Generator().manual_seed(7)).to(dev)
    for W in (2, 10):
        _never_fires(lambda: K.RnntBeamStream(w, 4, 64, W, blank=0), encj, T_LENS, 5, W, 23)


# ------------------------------------------------------------------------------------------------------------------ 5: the rule, against the oracle
CTC_SEEDS = (1, 6, 13)  # quiet / loud logits whose smallest oracle margin over every (W, H, C) below is >= 1e-3 (found on the CPU)


def _against_oracle(stream, feed, runs, W, H, what):
    """feed(i) advances the stream by chunk i -> the streams' frames in it; runs[b] = the oracle's run of stream b"""
    B = stream.B
    got, at = [[] for _ in range(B)], [0] * B
    i = 0
    while any(at[b] < len(runs[b]["steps"]) for b in range(B)):
        nv = feed(i)
        i += 1
        take(stream, got, horizon=H)
        rows, rest = full_beam(stream, W)
        scores = rest[0]
        for b in range(B):
            if nv[b] == 0:
                continue
            frames, committed, live = runs[b]["steps"][at[b]]
            at[b] += 1
            assert tuple(got[b]) == committed, (what, b, frames)
            assert rows[b] == [y for y, _ in live], (what, b, frames)
            np.testing.assert_allclose(scores[b, :len(live)].numpy(), [t for _, t in live], rtol=1e-3, atol=1e-3)
            assert int(stream.hstate[b, 0]) == frames
    worst = min(r["margin"] for r in runs)
    assert worst >= 1e-4, f"input condition: the oracle's smallest decision margin is {worst:.3g} (< 1e-4): choose other seeds"
    assert sum(r["horizon"].fired for r in runs) > 0, "input condition: some prune point removes a row"
    assert sum(r["horizon"].plain for r in runs) > 0, "input condition: some prune point leaves the common ancestor in charge"


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("H", [4, 16])
@pytest.mark.parametrize("W", [2, 4, 8])
def test_ctc_rule_against_the_oracle(dev, W, H, C):
    B, T, V, blank = 3, 60, 6, 5
    x = np.stack([HO.quiet_loud(np.random.default_rng(s), T, V, blank) for s in CTC_SEEDS])
    runs = [HO.ctc_stream(x[b], W, blank, C, H) for b in range(B)]
    xd = torch.from_numpy(x).to(dev)
    s = K.CtcBeamStream(B, C, T, V, W, blank_index=blank, device=dev)

    def feed(i):
        s.advance(xd[:, i * C:(i + 1) * C].contiguous(), [min(C, T - i * C)] * B)
        return [min(C, T - i * C)] * B

    _against_oracle(s, feed, runs, W, H, (W, H, C))


# (lengths in samples, signal seed): ContextNet on the signals of SEARCH_CASES; the Conformer's prune points remove no row on those (10
# frames at most), so it takes 18 to 25 frames of another seed.  Oracle margins of these, measured once: >= 1.4e-3.
RULE_SIGNALS = {"conformer": ([16000, 11300, 13700], 14), "contextnet": (LENS, 10)}


@pytest.mark.parametrize("kind", ["conformer", "contextnet"])
@pytest.mark.parametrize("W", [2, 4])
def test_transducer_rule_against_the_oracle(dev, kind, W):
    """the models of test_rnnt_beam_gpu.test_search_matches_oracle_on_tiny_models, chunks of 3 frames, horizon 4; the rows that leave
    take their token and prediction state with them: the survivors' continuations are the oracle's"""
    H, C = 4, 3
    mseed, _, bias = SEARCH_CASES[(kind, W)]
    model = sharpened(kind, dev, seed=mseed, blank_bias=bias)
    enc, elen = model.encode(*signals(*RULE_SIGNALS[kind])[:2])
    elen = [int(v) for v in elen]
    B = enc.shape[0]
    encj = K.matmul(enc.float().reshape(-1, enc.shape[2]).contiguous(), model.ps.p2d("joint/enc/w"), bias=model.ps.p("joint/enc/b"))
    encj = encj.view(B, enc.shape[1], -1)
    net = Net(model)
    ej = net.encj(enc.double().cpu().numpy())
    runs = [HO.rnnt_stream(net, ej[b, :n], W, model.blank, C, H) for b, n in enumerate(elen)]
    s = K.RnntBeamStream(model_weights(model), B, max(elen), W, blank=model.blank)

    def feed(i):
        nv = [min(max(n - i * C, 0), C) for n in elen]
        s.advance(chunk_of(encj, [i * C] * B, nv, C), nv)
        return nv

    _against_oracle(s, feed, runs, W, H, (kind, W))
    _, (scores, ntok, nh, nc) = full_beam(s, W)
    for b in range(B):
        for p, hy in enumerate(runs[b]["hyps"]):
            assert int(ntok[b, p]) == hy["tok"]
            np.testing.assert_allclose(nh[b, p].numpy(), hy["h"], rtol=1e-3, atol=1e-4)
            np.testing.assert_allclose(nc[b, p].numpy(), hy["c"], rtol=1e-3, atol=1e-4)


# ------------------------------------------------------------------------------------------------------------------ 6: past the capacity
def _past_capacity(make, x, W):
    """make(Tcap) -> a stream; x [2, 400, D].  Tcap = 32 with compactions against Tcap = 512 without, horizon 8, chunks of 4"""
    B, T, C, H, Tcap = 2, 400, 4, 8, 32
    small, big = make(Tcap), make(512)
    gs, gb = [[] for _ in range(B)], [[] for _ in range(B)]
    longest = compactions = 0
    for t0 in range(0, T, C):
        xc = x[:, t0:t0 + C].contiguous()
        over = [b for b in range(B) if small.frames[b] + C > Tcap]
        if over:
            small.compact(over)
            compactions += 1
        small.advance(xc, [C] * B)
        big.advance(xc, [C] * B)
        take(small, gs, horizon=H)
        take(big, gb, horizon=H)
        assert gs == gb, t0
        assert_same_beam(small, big, W, t0)
        assert small.hstate[:, 0].tolist() == [t0 + C] * B
        rows, _ = full_beam(big, W)
        longest = max(longest, max(len(y) - len(g) for r, g in zip(rows, gb) for y in r))
    assert big.frames == [T] * B and compactions > 1 and max(small.frames) <= Tcap
    assert longest + C <= Tcap, f"input condition: the longest uncommitted suffix ({longest}) plus a chunk fits the small trie"
    assert sum(len(g) for g in gs) > 0
    plain = make(Tcap)
    for t0 in range(0, Tcap, C):
        plain.advance(x[:, t0:t0 + C].contiguous(), [C] * B)
    with pytest.raises(RuntimeError, match="stream 0"):
        plain.advance(x[:, Tcap:Tcap + C].contiguous(), [C] * B)


CAPACITY_SEEDS = (41, 43)


@pytest.mark.parametrize("W", [2, 8])
def test_ctc_stream_runs_past_its_capacity(dev, W):
    """Input condition, asserted from the oracle: on these logits no sequence that a compaction dropped comes back young enough to move
    a horizon decision (the oracle run with the compactions of a Tcap = 32 stream equals the run without).  That is not so for every
    input: test_beam_horizon_oracle.test_a_compaction_makes_a_returning_sequence_young pins seed 40, where the compacted stream commits
    one label later from frame 260 on and this comparison fails at t0 = 256 (57 against 58 labels committed)."""
    V, blank = 6, 5
    x = np.stack([HO.quiet_loud(np.random.default_rng(s), 400, V, blank) for s in CAPACITY_SEEDS])
    for b in range(2):
        assert HO.ctc_stream(x[b], W, blank, 4, 8)["steps"] == HO.ctc_stream(x[b], W, blank, 4, 8, Tcap=32)["steps"], CAPACITY_SEEDS[b]
    x = torch.from_numpy(x).to(dev)
    _past_capacity(lambda Tcap: K.CtcBeamStream(2, 4, Tcap, V, W, blank_index=blank, device=dev), x, W)


@pytest.mark.parametrize("W", [2, 8])
def test_transducer_stream_runs_past_its_capacity(dev, W):
    w = rand_weights(dev, 29, 24, 24, 40, seed=17)
    encj = torch.randn(2, 400, 40, generator=torch.Generator().manual_seed(9)).to(dev)
    _past_capacity(lambda Tcap: K.RnntBeamStream(w, 2, Tcap, W, blank=0), encj, W)


# ------------------------------------------------------------------------------------------------------------------ 7: reset
def test_reset_of_one_stream_leaves_the_others_and_their_horizon_state_bit_equal(dev):
    V, E, U, J, W, C, B, H = 29, 24, 24, 40, 4, 5, 3, 5
    w = rand_weights(dev, V, E, U, J, seed=11)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 20, J, generator=g).to(dev)
    y = torch.randn(1, 10, J, generator=g).to(dev)  # the utterance that takes slot 1 after the reset
    s, whole, fresh = K.RnntBeamStream(w, B, 32, W), K.RnntBeamStream(w, B, 32, W), K.RnntBeamStream(w, 1, 32, W)
    for t0 in (0, 5):
        for r in (s, whole):
            r.advance(x[:, t0:t0 + C].contiguous(), [C, C, C])
            r.commit(horizon=H)
    s.compact([1])
    before, state = s.nbest(W), s.hstate.clone()
    s.reset(rows=[1])
    for p, q in zip(before, s.nbest(W)):
        assert torch.equal(p[0], q[0]) and torch.equal(p[2], q[2])
    assert torch.equal(s.hstate[0], state[0]) and torch.equal(s.hstate[2], state[2]) and not s.hstate[1].any()
    assert s.frames == [10, 0, 10] and int(s.committed[1]) == 0 and s.dropped[1] == []
    assert rows_of(*s.nbest(W)[:3])[1] == [()]
    for t0 in (10, 15):
        z = x[:, t0:t0 + C].clone()
        z[1] = y[0, t0 - 10:t0 - 10 + C]
        s.advance(z, [C, C, C])
        whole.advance(x[:, t0:t0 + C].contiguous(), [C, C, C])
        fresh.advance(y[:, t0 - 10:t0 - 10 + C].contiguous(), [C])
        for r in (s, whole, fresh):
            r.commit(horizon=H)
    for a, f_, o in zip(s.nbest(W), whole.nbest(W), fresh.nbest(W)):
        for b in (0, 2):
            assert torch.equal(a[b], f_[b])
        if a.dtype == torch.int32 and a.dim() == 3:
            assert torch.equal(a[1, :, :10], o[0]) and (a[1, :, 10:] == 0).all()
        else:
            assert torch.equal(a[1], o[0])
    assert torch.equal(s.hstate[0], whole.hstate[0]) and torch.equal(s.hstate[2], whole.hstate[2]) and torch.equal(s.hstate[1], fresh.hstate[0])
    assert torch.equal(s.committed.cpu(), torch.cat([whole.committed[:1], fresh.committed, whole.committed[2:]]).cpu())
