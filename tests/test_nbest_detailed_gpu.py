"""recognize_nbest_detailed on tiny models (random weights): the search part is recognize_nbest / recognize_nbest_lm bit for bit, the
details of every hypothesis are what a forced alignment of that hypothesis gives (K.ctc_align / model.align for CTC, align_encoded for
the transducer), dead paths stay marked, and NBestOutput.path feeds token_times / token_confidences / word_details.  The transducer's
entropies are held to f64 entropies of the model's own f32 joint, within twice the error recognize_detailed's entropies show against
the same kind of reference on the same model (recorded in profiles/nbest_detail_parity.json)."""
import os

import numpy as np
import pytest
import torch

import nbest_detail_oracle as O
from tensorflowasr_amd import configs, schemas
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import tokenizers as tk
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.ctc_model import ConformerCTC
from tensorflowasr_amd.lm import NGramLM
from tensorflowasr_amd.schemas import NBestOutput, PredictInput, TrainData, TrainInput, TrainLabel

pytestmark = pytest.mark.gpu
I32 = torch.int32
NEG = float("-inf")
LENS = [6400, 4000, 5200]
VOCAB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "librispeech", "characters", "english.vocab")


def signals(lens, seed):
    rng = np.random.default_rng(seed)
    sig = np.clip(rng.standard_normal((len(lens), max(lens))) * 0.1, -1, 1).astype(np.float32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0.0
    return PredictInput(torch.from_numpy(sig), torch.tensor(lens, dtype=I32))


@pytest.fixture(scope="module")
def ctc(dev):
    model = ConformerCTC(configs.conformer_tiny(head="ctc"), dev, dtype=torch.float32, seed=2)
    with torch.no_grad():
        model.ps.p("dec/logits/w").mul_(3.0)
    model.ps.refresh_shadow()
    return model


def check_surface(out, model, B, P):
    assert isinstance(out, NBestOutput)
    W = out.tokens.shape[2]
    assert out.tokens.shape == (B, P, W) and out.lengths.shape == (B, P) and out.path_scores.shape == (B, P)
    for t in (out.frames, out.log_probs, out.entropies) + (() if out.ends is None else (out.ends,)):
        assert t.shape == (B, P, W)
    assert out.seconds_per_frame == pytest.approx(model.seconds_per_frame) and out.vocab_size == model.cfg.vocab_size
    none = out.frames < 0
    assert (out.log_probs[none] == 0).all() and (out.entropies[none] == 0).all()
    cols = torch.arange(W, device=out.frames.device).view(1, 1, W)
    live = torch.isfinite(out.path_scores).unsqueeze(2)
    assert torch.equal(~none, live & (cols < out.lengths.unsqueeze(2)))  # a token of an aligned path has a frame, nothing else has
    assert (out.entropies >= 0).all() and (out.entropies <= np.log(model.cfg.vocab_size) + 1e-5).all()


def test_ctc_plain_search(ctc):
    inputs = signals(LENS, 11)
    W, P = 6, 4
    out = ctc.recognize_nbest_detailed(inputs, beam_width=W, top_paths=P)
    out = out._replace(**{k: v.clone() for k, v in out._asdict().items() if torch.is_tensor(v)})
    ref = ctc.recognize_nbest(inputs, beam_width=W, top_paths=P)
    assert len(out.search) == 3 and all(torch.equal(a, b) for a, b in zip(out.search, ref))
    assert torch.equal(out.tokens, ref[0]) and torch.equal(out.lengths, ref[1])
    check_surface(out, ctc, len(LENS), P)
    logits, elen = ctc._infer_logits(inputs)
    V = ctc.cfg.vocab_size
    assert torch.isfinite(ref[2]).all() and (ref[1] > 0).any()
    for p in range(P):
        start, end, lp, score = K.ctc_align(logits, ref[0][:, p].contiguous(), ref[1][:, p].contiguous(), ctc._h2d(elen), blank=V - 1)
        assert torch.equal(out.frames[:, p], start) and torch.equal(out.ends[:, p], end)
        assert torch.equal(out.log_probs[:, p], lp) and torch.equal(out.path_scores[:, p], score)


def test_ctc_lm_search(ctc):
    inputs = signals(LENS, 12)
    V, blank = ctc.cfg.vocab_size, int(ctc.blank)
    rng = np.random.default_rng(5)
    lm = NGramLM.estimate([rng.integers(1, V, int(rng.integers(2, 9))).tolist() for _ in range(200)], 2, V, blank)
    W, P = 5, 3
    out = ctc.recognize_nbest_detailed(inputs, beam_width=W, top_paths=P, lm=lm, alpha=0.4, beta=0.3)
    out = out._replace(**{k: v.clone() for k, v in out._asdict().items() if torch.is_tensor(v)})
    ref = ctc.recognize_nbest_lm(inputs, lm, beam_width=W, top_paths=P, alpha=0.4, beta=0.3)
    assert len(out.search) == 5 and all(torch.equal(a, b) for a, b in zip(out.search, ref))
    check_surface(out, ctc, len(LENS), P)
    assert torch.isfinite(ref[2]).all()
    for p in range(P):
        labels = ref[0][:, p].cpu()
        data = TrainData(TrainInput(inputs.inputs, inputs.inputs_length, torch.zeros(len(LENS), 1, dtype=I32), torch.ones(len(LENS), dtype=I32)),
                         TrainLabel(labels, ref[1][:, p].cpu()))
        a = ctc.align(data)
        assert torch.equal(out.frames[:, p], a.frames) and torch.equal(out.ends[:, p], a.ends)
        assert torch.equal(out.log_probs[:, p], a.label_log_probs) and torch.equal(out.path_scores[:, p], a.scores)
    with pytest.raises(ValueError):
        ctc.recognize_nbest_detailed(inputs, lm=NGramLM.estimate([[1, 2]], 2, V + 1, blank))


def test_ctc_dead_paths_stay_marked(ctc, monkeypatch):
    """One frame leaves vocab_size live beams (the empty prefix and one per label): asking for more paths than that returns dead ones,
    empty with search score -inf.  An empty label row would align (the all-blank path): the mark keeps it out."""
    inputs = signals(LENS, 13)
    real = ctc._infer_logits
    monkeypatch.setattr(ctc, "_infer_logits", lambda x: (lambda lg, n: (lg, [n[0], 1, n[2]]))(*real(x)))
    V = ctc.cfg.vocab_size
    P = V + 3
    out = ctc.recognize_nbest_detailed(inputs, beam_width=P, top_paths=P)
    check_surface(out, ctc, len(LENS), P)
    score = out.search[2]
    dead = score == NEG
    assert dead[1].sum() == 3 and not dead[1, :V].any() and (out.lengths[dead] == 0).all()
    assert (out.path_scores[dead] == NEG).all() and (out.frames[dead] == -1).all() and (out.ends[dead] == -1).all()
    assert torch.isfinite(out.path_scores[1, :V]).all()  # the empty prefix among them: a live path without labels does align
    assert ((out.lengths[1, :V] == 0).sum() == 1)


def test_path_feeds_the_schema_helpers(ctc):
    inputs = signals(LENS, 11)
    out = ctc.recognize_nbest_detailed(inputs, beam_width=6, top_paths=4)
    t = tk.get({"type": "characters", "blank_index": 0, "vocabulary": VOCAB})
    for p in (0, 3):
        one = out.path(p)
        assert isinstance(one, schemas.RecognizeOutput) and torch.equal(one.predict.tokens, out.tokens[:, p]) and torch.equal(one.scores, out.path_scores[:, p])
        times = schemas.token_times(one)
        assert torch.equal(times >= 0, one.frames >= 0)
        np.testing.assert_allclose(times[one.frames >= 0].cpu().numpy(), one.frames[one.frames >= 0].cpu().numpy() * out.seconds_per_frame, rtol=1e-6)
        for method in ("prob", "entropy"):
            conf = schemas.token_confidences(one, method)
            assert (conf >= 0).all() and (conf <= 1 + 1e-6).all() and (conf[one.frames < 0] == 0).all() and (conf[one.frames >= 0] > 0).all()
        for b in range(len(LENS)):
            words = schemas.word_details(one, t, b)
            spans = [s for s in t.word_spans(one.predict.tokens[b].cpu().numpy()) if any(int(one.frames[b, k]) >= 0 for k in range(s[1], s[2] + 1))]
            assert [w[0] for w in words] == [s[0] for s in spans]
            for (word, s0, s1, lp, conf), (_, first, last) in zip(words, spans):
                cols = [k for k in range(first, last + 1) if int(one.frames[b, k]) >= 0]
                assert s0 == pytest.approx(int(one.frames[b, cols[0]]) * out.seconds_per_frame) and s0 < s1 and 0 < conf <= 1
                assert s1 == pytest.approx(int(one.ends[b, cols[-1]]) * out.seconds_per_frame)
                assert lp == pytest.approx(float(one.log_probs[b, cols].sum()), rel=1e-5, abs=1e-6)


# ------------------------------------------------------------------------------------------------------------------ transducer
@pytest.fixture(scope="module")
def rnnt(dev):
    model = ConformerTransducer(configs.conformer_tiny(), dev, dtype=torch.float32, seed=1)
    with torch.no_grad():
        model.ps.p("joint/vocab/w").mul_(3.0)
        model.ps.p("pred/emb").mul_(3.0)
    model.ps.refresh_shadow()
    return model


def f64_node_entropy(model, sig, slen, tokens, lengths, frames):
    """entropy in f64 of the model's own f32 joint output at the emitting node (frames[r, u], u) of every token"""
    R, U = tokens.shape
    preds = torch.cat([torch.zeros(R, 1, dtype=I32), tokens.cpu().to(I32)], 1)
    out = model(TrainInput(sig, slen, preds, (lengths.cpu() + 1).to(I32)))
    _, ent = O.frame_stats(out.logits.double().cpu().numpy())  # [R, T, U + 1]
    fr = frames.cpu().numpy()
    want = np.zeros((R, U))
    for r in range(R):
        for u in range(U):
            if fr[r, u] >= 0:
                want[r, u] = ent[r, fr[r, u], u]
    return want


def test_transducer(rnnt):
    model, dev = rnnt, rnnt.device
    inputs = signals(LENS, 21)
    B, W, P = len(LENS), 4, 3
    out = model.recognize_nbest_detailed(inputs, beam_width=W, top_paths=P)
    ref = model.recognize_nbest(inputs, beam_width=W, top_paths=P)
    assert len(out.search) == 3 and all(torch.equal(a, b) for a, b in zip(out.search, ref))
    assert out.ends is None and torch.equal(out.tokens, ref[0])
    check_surface(out, model, B, P)
    live = torch.isfinite(ref[2])
    assert live[:, 0].all() and int(ref[1].max()) > 0, "the search emitted nothing: the case shows nothing"
    # frames / log_probs: align_encoded row by row
    enc, elen = model.encode(inputs.inputs, inputs.inputs_length)
    R, U = B * P, int(ref[1].max())
    n = ref[1].reshape(R).clamp(min=0)
    lab = ref[0].reshape(R, -1)[:, :U].contiguous()
    a = model.align_encoded(enc.repeat_interleave(P, 0), [int(v) for v in elen for _ in range(P)],
                            torch.cat([torch.full((R, 1), model.blank, dtype=I32, device=dev), lab], 1), lab, n.cpu())
    rows = live.reshape(R)
    assert torch.equal(out.frames.reshape(R, -1)[rows, :U], a.frames[rows]) and torch.equal(out.log_probs.reshape(R, -1)[rows, :U], a.label_log_probs[rows])
    assert torch.equal(out.path_scores.reshape(R)[rows], a.scores[rows])
    assert (out.path_scores.reshape(R)[~rows] == NEG).all() and (out.frames.reshape(R, -1)[~rows] == -1).all()
    assert (out.frames[:, :, U:] == -1).all()
    # entropies: the parent's recognize_detailed against f64 of the model's own joint, utterance by utterance, sets the bound
    parent = 0.0
    tokens_seen = 0
    for b, m in enumerate(LENS):
        one = PredictInput(inputs.inputs[b:b + 1, :m].clone(), torch.tensor([m], dtype=I32))
        g = model.recognize_detailed(one)
        cols = (g.frames[0] >= 0).nonzero().reshape(-1)
        if len(cols) == 0:
            continue
        assert cols.tolist() == list(range(len(cols)))  # a single utterance: symbols from column 0
        toks = g.predict.tokens[:1, :len(cols)]
        want = f64_node_entropy(model, one.inputs, one.inputs_length, toks, torch.tensor([len(cols)]), g.frames[:1, :len(cols)])
        parent = max(parent, float(np.abs(g.entropies[0, :len(cols)].double().cpu().numpy() - want[0]).max()))
        tokens_seen += len(cols)
    assert tokens_seen > 0 and parent > 0
    sig_r, len_r = inputs.inputs.repeat_interleave(P, 0), inputs.inputs_length.repeat_interleave(P, 0)
    want = f64_node_entropy(model, sig_r, len_r, lab, n, out.frames.reshape(R, -1)[:, :U])
    mine = float(np.abs(out.entropies.reshape(R, -1)[:, :U].double().cpu().numpy() - want).max())
    fig = dict(parent_recognize_detailed_entropy=parent, parent_tokens=tokens_seen, new_entropy=mine, new_tokens=int((out.frames >= 0).sum()),
               bound_entropy=2 * parent)
    print("transducer n-best entropies:", fig)
    O.write_parity("transducer_nbest_entropy", fig)
    assert mine <= 2 * parent, fig
    # the helpers read a transducer path too
    one = out.path(0)
    assert one.ends is None and torch.equal(schemas.token_times(one) >= 0, one.frames >= 0)
    conf = schemas.token_confidences(one)
    assert (conf[one.frames >= 0] > 0).all() and (conf <= 1 + 1e-6).all()


def test_transducer_refuses_previous_tokens_and_states(rnnt):
    inputs = signals(LENS[:1], 22)
    with pytest.raises(ValueError):
        rnnt.recognize_nbest_detailed(inputs._replace(previous_tokens=torch.ones(1, 1, dtype=I32)))
    with pytest.raises(ValueError):
        rnnt.recognize_nbest_detailed(inputs._replace(previous_decoder_states=rnnt.get_initial_decoder_states(1)))
