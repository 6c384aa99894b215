"""tfasr_rnnt_beam_search: the device transducer beam search ("modified beam search": one symbol per frame at most, equal label
sequences merged) against a numpy oracle written here.  The selection is judged exactly through the test seam (caller-supplied
logits, the oracle's pinned arithmetic), the whole search on the tiny models' own encoder output (oracle in f64), and at W = 1
against the greedy search."""
import itertools

import numpy as np
import pytest
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.contextnet import ContextNetTransducer
from tensorflowasr_amd.schemas import PredictInput

pytestmark = pytest.mark.gpu
NEG = -np.inf


# ------------------------------------------------------------------------------------------------------------------ the oracle
def lae(a, b):
    """log(exp(a) + exp(b)) as the device computes it (f64)"""
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + np.log1p(np.exp(-abs(a - b)))


def pinned_lp(x):
    """log-probabilities of one f32 logit row with the search's pinned arithmetic: f32 max, f64 sum of exp, f32 log-sum-exp, f64 lp"""
    x = np.asarray(x, np.float32)
    m = np.float32(x.max())
    s = np.sum(np.exp(x.astype(np.float64) - np.float64(m)))
    lz = np.float32(m + np.float32(np.log(s)))
    return x.astype(np.float64) - np.float64(lz)


def beam_step(beam, lps, blank, W):
    """One frame of the modified beam search.  beam: [(label tuple, total)] best first; lps: [V] f64 log-probabilities per hypothesis.
    -> (next beam [(seq, total, src, label)] with label -1 = the stay (or merge) of row src, merges, margin at the cut or None)"""
    index = {y: i for i, (y, _) in enumerate(beam)}
    lp = np.stack(lps)
    tots = np.array([s for _, s in beam])[:, None] + lp
    valid = np.ones(tots.shape, bool)
    valid[:, blank] = False
    stay = {y: [s + lp[i, blank], i] for i, (y, s) in enumerate(beam)}
    merges = 0
    for j, (y, _) in enumerate(beam):
        if y and y[:-1] in index:
            p = index[y[:-1]]
            stay[y][0] = lae(tots[p, y[-1]], stay[y][0])
            valid[p, y[-1]] = False
            merges += 1
    rows, cols = np.nonzero(valid & (tots != NEG))
    et = tots[rows, cols]
    st = np.array([v[0] for v in stay.values()])
    allt = np.concatenate([st, et])
    n = len(allt)
    thr = -np.partition(-allt, W)[W] if n > W else -np.inf
    cands = [(v[0], y, v[1], -1) for y, v in stay.items() if v[0] >= thr]
    keep = et >= thr
    cands += [(t, beam[p][0] + (int(c),), int(p), int(c)) for t, p, c in zip(et[keep], rows[keep], cols[keep])]
    cands.sort(key=lambda c: (-c[0], c[1]))
    margin = cands[W - 1][0] - cands[W][0] if n > W else None
    return [(y, t, src, lab) for t, y, src, lab in cands[:W]], merges, margin


def final_gap(beam):
    t = [s for _, s in beam]
    return min((a - b for a, b in zip(t, t[1:])), default=None)


# ------------------------------------------------------------------------------------------------------------------ seam helpers
def nbest_rows(seam):
    toks, lens, sc = (x.cpu().numpy() for x in seam.nbest())
    return [[(tuple(toks[b, i, :lens[b, i]].tolist()), float(sc[b, i])) for i in range(toks.shape[1])] for b in range(toks.shape[0])]


def assert_beam_equal(dev_rows, beam, W, what):
    assert len(dev_rows) == W
    for i, (y, s) in enumerate(dev_rows):
        if i < len(beam):
            assert y == beam[i][0], (what, i, y, beam[i][0])
            np.testing.assert_allclose(s, np.float32(beam[i][1]), rtol=1e-6, atol=1e-6, err_msg=f"{what} row {i}")
        else:
            assert y == () and s == NEG, (what, i, y, s)


def run_seam(x, nframes, W, blank, init=None):
    """x [B,T,W,V] f32 logits of the beam rows per frame -> per-frame device beams checked against the oracle; returns merges"""
    B, T, _, V = x.shape
    seam = K.rnnt_beam_begin(B, T, V, W, blank, init_tok=init)
    beams = [[((), 0.0)] for _ in range(B)]
    merges = 0
    nf = torch.tensor(nframes, dtype=torch.int32)
    for t in range(T):
        seam.select(torch.from_numpy(x[:, t]).cuda(), nf, t)
        for b in range(B):
            if t < nframes[b]:
                nxt, m, _ = beam_step(beams[b], [pinned_lp(x[b, t, i]) for i in range(len(beams[b]))], blank, W)
                beams[b] = [(y, s) for y, s, _, _ in nxt]
                merges += m
        rows = nbest_rows(seam)
        for b in range(B):
            assert_beam_equal(rows[b], beams[b], W, f"t={t} b={b}")
    return merges


# ------------------------------------------------------------------------------------------------------------------ 1-4: the seam
@pytest.mark.parametrize("V", [3, 29, 1000])
def test_selection_matches_oracle_frame_by_frame(dev, V):
    rng = np.random.default_rng(V)
    nframes = [7, 0, 1, 5, 7, 3]
    for W in (1, 2, 4, 10, 16, 64):
        for blank in (0, V - 1):
            x = (rng.standard_normal((len(nframes), 7, W, V)) * (1.0, 2.0, 4.0)[W % 3]).astype(np.float32)
            run_seam(x, nframes, W, blank)


def test_exact_ties_follow_label_order(dev):
    rng = np.random.default_rng(1)
    V, T = 29, 6
    for W in (2, 4, 10):
        x = (rng.standard_normal((3, T, W, V)) * 2).astype(np.float32)
        x[0, :, :, 5] = x[0, :, :, 3]  # duplicated columns: equal extensions of one row
        x[0, :, :, 9] = x[0, :, :, 3]
        x[1] = 0.5  # flat rows: every candidate of a row ties with its stay
        x[2, ::2, :, :] = x[2, ::2, :1, :]  # every row of the frame has the same logits: totals tie across rows
        run_seam(x, [T, T, T], W, 0)
        run_seam(x, [T, T, T], W, V - 1)


def test_merges_happen_and_are_right(dev):
    rng = np.random.default_rng(3)
    for W in (2, 3):
        x = (rng.standard_normal((4, 40, W, 3)) * 1.5).astype(np.float32)
        merges = run_seam(x, [40, 40, 33, 17], W, 0)
        assert merges > 10, merges


def test_wide_beam_is_exact_nbest(dev):
    """A prefix-dependent fake model (logits keyed by (t, label prefix)); W = 64 holds every sequence of T <= 5 frames over V = 3,
    so the n-best list is the exact distribution over label sequences of all one-symbol-per-frame alignments."""
    V, W, blank = 3, 64, 0
    for T, seed in ((3, 0), (5, 1)):
        rng = np.random.default_rng(seed)
        table = {}

        def row(t, y):
            if (t, y) not in table:
                table[(t, y)] = (rng.standard_normal(V) * 1.5).astype(np.float32)
            return table[(t, y)]

        seam = K.rnnt_beam_begin(1, T, V, W, blank)
        nf = torch.tensor([T], dtype=torch.int32)
        for t in range(T):
            rows = nbest_rows(seam)[0]
            x = np.zeros((1, W, V), np.float32)
            for i, (y, s) in enumerate(rows):
                if s != NEG:
                    x[0, i] = row(t, y)
            seam.select(torch.from_numpy(x).cuda(), nf, t)
        # brute force: every alignment (blank or one label per frame), summed per label sequence
        paths = {}
        for choice in itertools.product(range(V), repeat=T):
            y, s = (), 0.0
            for t, c in enumerate(choice):
                s += pinned_lp(row(t, y))[c]
                if c != blank:
                    y = y + (c,)
            paths[y] = lae(paths.get(y, NEG), s)
        want = sorted(paths.items(), key=lambda kv: (-kv[1], kv[0]))
        got = nbest_rows(seam)[0]
        assert len(want) < W
        for i, (y, s) in enumerate(got):
            if i < len(want):
                assert y == want[i][0], (T, i, y, want[i][0])
                np.testing.assert_allclose(s, want[i][1], rtol=1e-6, err_msg=f"T={T} path {i}")
            else:
                assert y == () and s == NEG


# ------------------------------------------------------------------------------------------------------------------ models
def sharpened(kind, dev, dtype=torch.float32, seed=0, blank_bias=0.0, gain=3.0):
    """tiny model with a peaky joint (vocabulary projection x gain) and a token-sensitive prediction network (embedding x gain):
    the search's decisions are far from ties"""
    if kind == "conformer":
        model = ConformerTransducer(configs.conformer_tiny(), dev, dtype=dtype, seed=seed)
    else:
        model = ContextNetTransducer(configs.contextnet_tiny(), dev, dtype=dtype, seed=seed)
    with torch.no_grad():
        model.ps.p("joint/vocab/w").mul_(gain)
        model.ps.p("pred/emb").mul_(gain)
        model.ps.p("joint/vocab/b")[0] += blank_bias
    model.ps.refresh_shadow()
    return model


def signals(lens, seed):
    rng = np.random.default_rng(seed)
    sig = np.clip(rng.standard_normal((len(lens), max(lens))) * 0.1, -1, 1).astype(np.float32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0.0
    return PredictInput(torch.from_numpy(sig), torch.tensor(lens, dtype=torch.int32))


class Net:
    """the prediction + joint network in f64 (oracle.conformer_ref._call_next), on the model's f32 master weights"""

    def __init__(self, model):
        W = {k: v.double().numpy() for k, v in model.ps.export_keras().items() if k.startswith(("pred/", "joint/"))}
        self.W, self.ln = W, model.cfg.prediction_layer_norm

    def step(self, tok, h, c):
        W = self.W
        z = W["pred/emb"][tok] @ W["pred/lstm/k"] + h @ W["pred/lstm/rk"] + W["pred/lstm/b"]
        i, f, g, o = np.split(z, 4)
        sg = lambda v: 1.0 / (1.0 + np.exp(-v))
        cn = sg(f) * c + sg(i) * np.tanh(g)
        hn = sg(o) * np.tanh(cn)
        y = hn
        if self.ln:
            mu = y.mean()
            y = (y - mu) / np.sqrt(((y - mu) ** 2).mean() + 1e-3) * W["pred/ln/g"] + W["pred/ln/b"]
        return hn, cn, y @ W["joint/pred/w"] + W["joint/pred/b"]

    def encj(self, enc):
        return enc @ self.W["joint/enc/w"] + self.W["joint/enc/b"]

    def logp(self, ej, pred):
        x = np.tanh(ej + pred) @ self.W["joint/vocab/w"] + self.W["joint/vocab/b"]
        m = x.max()
        return x - (m + np.log(np.exp(x - m).sum()))


def model_oracle(net, ej, W, blank, tok0=0, h0=None, c0=None):
    """f64 modified beam search of one utterance on its joint encoder projection ej [n, J] -> (final [(seq, total, tok, h, c)], margins)"""
    U = net.W["pred/lstm/rk"].shape[0]
    h0 = np.zeros(U) if h0 is None else h0
    c0 = np.zeros(U) if c0 is None else c0
    hyps = [dict(seq=(), tot=0.0, tok=tok0, h=h0, c=c0, post=net.step(tok0, h0, c0))]
    margins = []
    for t in range(len(ej)):
        lps = [net.logp(ej[t], hy["post"][2]) for hy in hyps]
        nxt, _, margin = beam_step([(hy["seq"], hy["tot"]) for hy in hyps], lps, blank, W)
        if margin is not None:
            margins.append(margin)
        new = []
        for y, tot, src, lab in nxt:
            if lab < 0:
                new.append(dict(hyps[src], seq=y, tot=tot))
            else:
                hp, cp, _ = hyps[src]["post"]
                new.append(dict(seq=y, tot=tot, tok=lab, h=hp, c=cp, post=net.step(lab, hp, cp)))
        hyps = new
    gap = final_gap([(hy["seq"], hy["tot"]) for hy in hyps])
    if gap is not None:
        margins.append(gap)
    return hyps, margins


# (model, beam width) -> (model seed, signal seed, blank bias): fixed, the blank bias raised until paths mix blanks and labels; the
# oracle's smallest margin (>= 1e-3 for these) is asserted below
SEARCH_CASES = {("conformer", 2): (0, 10, 4.0), ("conformer", 4): (0, 10, 4.0), ("conformer", 8): (0, 10, 4.0),
                ("contextnet", 2): (3, 10, 2.0), ("contextnet", 4): (3, 10, 2.0), ("contextnet", 8): (3, 10, 2.0)}
LENS = [6400, 3700, 5100]
MIXED = 4.0  # conformer_tiny seed 0: blank bias at which the paths mix blanks and labels


def search_case(kind, W, dev):
    mseed, sseed, bias = SEARCH_CASES[(kind, W)]
    model = sharpened(kind, dev, seed=mseed, blank_bias=bias)
    enc, elen = model.encode(*signals(LENS, sseed)[:2])
    toks, lens, scores, ntok, states = (x.cpu() for x in model.recognize_beam_encoded(enc, elen, W, W))
    net = Net(model)
    ej = net.encj(enc.double().cpu().numpy())
    worst = np.inf
    for b, n in enumerate(elen):
        hyps, margins = model_oracle(net, ej[b, :n], W, model.blank)
        worst = min([worst] + margins)
        for p in range(W):
            if p < len(hyps):
                hy = hyps[p]
                assert int(lens[b, p]) == len(hy["seq"]) and tuple(toks[b, p, :lens[b, p]].tolist()) == hy["seq"], (kind, W, b, p)
                assert (toks[b, p, lens[b, p]:] == model.blank).all()
                np.testing.assert_allclose(float(scores[b, p]), hy["tot"], rtol=1e-3, atol=1e-3)
                assert int(ntok[b, p]) == hy["tok"]
                np.testing.assert_allclose(states[b, p, 0, 0].numpy(), hy["h"], rtol=1e-3, atol=1e-4)
                np.testing.assert_allclose(states[b, p, 0, 1].numpy(), hy["c"], rtol=1e-3, atol=1e-4)
            else:
                assert int(lens[b, p]) == 0 and float(scores[b, p]) == NEG
    return worst


@pytest.mark.parametrize("kind", ["conformer", "contextnet"])
@pytest.mark.parametrize("W", [2, 4, 8])
def test_search_matches_oracle_on_tiny_models(dev, kind, W):
    worst = search_case(kind, W, dev)
    assert worst >= 1e-4, f"the fixed seeds of {kind} W={W} leave a margin of {worst:.3g} (< 1e-4): choose others"


# ------------------------------------------------------------------------------------------------------------------ 5: W = 1
def test_width_one_equals_greedy(dev):
    model = sharpened("conformer", dev, seed=0, blank_bias=MIXED)
    inp = signals([6400], 21)
    g = model.recognize(inp, max_tokens_per_frame=1)
    bm = model.recognize_beam(inp, beam_width=1, device_search=True)
    n = g.tokens.shape[1]
    assert (g.tokens != model.blank).any(), "the greedy search emits nothing: raise the margins"
    np.testing.assert_array_equal(bm.tokens[:, :n].cpu().numpy(), g.tokens.cpu().numpy())
    assert (bm.tokens[:, n:] == model.blank).all()
    np.testing.assert_array_equal(bm.next_tokens.cpu().numpy(), g.next_tokens.cpu().numpy())
    np.testing.assert_allclose(bm.next_decoder_states.cpu().numpy(), g.next_decoder_states.cpu().numpy(), rtol=1e-4, atol=1e-5)
    # a ragged batch in one call == the greedy search of each utterance alone, on the same encoder output
    enc, elen = model.encode(*signals([6400, 3700, 5100], 22)[:2])
    toks, lens, _, ntok, states = model.recognize_beam_encoded(enc, elen, 1, 1)
    for b, n in enumerate(elen):
        g = model.recognize_encoded(enc[b:b + 1, :n].contiguous(), [n], max_tokens_per_frame=1)
        gt = g.tokens[0].cpu().numpy()
        emitted = gt[gt != model.blank]
        assert int(lens[b, 0]) == len(emitted) and toks[b, 0, :len(emitted)].cpu().numpy().tolist() == emitted.tolist(), b
        assert int(ntok[b, 0]) == int(g.next_tokens[0, 0])
        np.testing.assert_allclose(states[b, 0].cpu().numpy(), g.next_decoder_states[0].cpu().numpy(), rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------------------------------------------------------ 7, 8, 10
def test_bf16_model_searches_on_its_f32_twin(dev):
    m32 = sharpened("conformer", dev, seed=0, blank_bias=MIXED)
    m16 = ConformerTransducer(configs.conformer_tiny(), dev, dtype=torch.bfloat16, seed=5)
    m16.ps.import_keras(m32.ps.export_keras())
    inp = signals(LENS, 10)
    a = [x.cpu() for x in m32.recognize_nbest(inp, beam_width=4, top_paths=4)]
    b = [x.cpu() for x in m16.recognize_nbest(inp, beam_width=4, top_paths=4)]
    np.testing.assert_array_equal(a[0].numpy(), b[0].numpy())
    np.testing.assert_array_equal(a[1].numpy(), b[1].numpy())
    np.testing.assert_allclose(a[2].numpy(), b[2].numpy(), rtol=1e-5)


def test_continuation_equals_one_search(dev):
    model = sharpened("conformer", dev, seed=0, blank_bias=MIXED)
    enc, elen = model.encode(*signals([6400], 23)[:2])
    T = elen[0]
    t1 = T // 2
    full = model.recognize_beam_encoded(enc[:, :T].contiguous(), [T], 1, 1)
    a = model.recognize_beam_encoded(enc[:, :t1].contiguous(), [t1], 1, 1)
    b = model.recognize_beam_encoded(enc[:, t1:T].contiguous(), [T - t1], 1, 1, previous_tokens=a[3][:, :1],
                                     previous_decoder_states=a[4][:, 0])
    joined = a[0][0, 0, :int(a[1][0, 0])].tolist() + b[0][0, 0, :int(b[1][0, 0])].tolist()
    assert joined == full[0][0, 0, :int(full[1][0, 0])].tolist()
    assert int(b[3][0, 0]) == int(full[3][0, 0])
    np.testing.assert_array_equal(b[4].cpu().numpy(), full[4].cpu().numpy())
    np.testing.assert_allclose(float(a[2][0, 0]) + float(b[2][0, 0]), float(full[2][0, 0]), rtol=1e-5)


def test_default_recognize_beam_is_still_greedy(dev):
    model = sharpened("conformer", dev, seed=0, blank_bias=MIXED)
    inp = signals(LENS, 24)
    np.testing.assert_array_equal(model.recognize_beam(inp).tokens.cpu().numpy(), model.recognize(inp).tokens.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ 9: bench shape
def test_bench_shape_is_deterministic_and_ordered(dev):
    g = torch.Generator().manual_seed(0)
    B, T, E, U, J, V = 32, 250, 640, 640, 640, 1000
    r = lambda *s, fan: (torch.randn(*s, generator=g) / fan ** 0.5).to(dev)
    emb, wk, wrk, b = r(V, E, fan=1), r(E, 4 * U, fan=E), r(U, 4 * U, fan=U), r(4 * U, fan=4)
    lng, lnb = 1 + 0.1 * r(U, fan=1), 0.1 * r(U, fan=1)
    wjp, bjp, wv, bv = r(U, J, fan=U), r(J, fan=4), r(J, V, fan=J / 4), r(V, fan=1)
    encj = r(B, T, J, fan=1)
    nframes = torch.tensor([T - 3 * i for i in range(B)], dtype=torch.int32)
    packed = K.decode_pack(emb, wk, wrk, wjp, wv)
    assert packed is not None
    for W in (4, 10):
        runs = [K.rnnt_beam_search(emb, wk, wrk, b, lng, lnb, wjp, bjp, wv, bv, encj, nframes, W, 4, 0, packed=pk)
                for pk in (None, None, packed)]
        runs = [[x.cpu() for x in run] for run in runs]
        for other in runs[1:]:  # bit-identical, with G from the search's own product or from decode_pack
            for x, y in zip(runs[0], other):
                assert torch.equal(x, y)
        toks, lens, sc = runs[0][:3]
        assert (sc[:, 1:] <= sc[:, :-1]).all()
        assert (lens <= nframes[:, None]).all() and torch.isfinite(sc[:, 0]).all()
        assert (lens[:, 0] > 0).any()
