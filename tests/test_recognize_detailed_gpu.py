"""recognize_detailed through the models.

Transducer: the whole greedy search with the detail bookkeeping on both routes of recognize_encoded (the fused decode_steps route at
B = 17, the per-op loop at B = 65, the single-utterance search at B = 1), with the weights and inputs of
tests/test_decode_step_gpu.py's search_case.  Tokens, next_tokens and the decoder states are bit-equal to recognize_encoded; frames are
exactly those of the float64 search of tests/recognize_detail_oracle.py; log_probs and entropies meet the whole-step bar of that file
(rtol 1e-3 / atol 1e-4: the logits now come from the device).  The test asserts again, from the float64 search, that no decision had a
top-2 margin under 1e-3.

CTC: a cross-check of two independent kernels.  The frame-wise arg-max path is the most probable path overall, hence the best path of
its own labelling: model.align on the tokens of recognize_detailed must return the same spans exactly and the same log-probabilities
within the summed single-layer bar (n atol + rtol |value|, rtol 1e-4 / atol 1e-5).  Viterbi ties are excluded on the host first: every
frame's top-2 log-probability margin must exceed 1e-3 (the first seed of a short list that meets it is used)."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.ctc_model import ConformerCTC
from tensorflowasr_amd.schemas import PredictInput, RecognizeOutput, TrainData, TrainInput, TrainLabel, token_confidences, token_times

import recognize_detail_oracle as RD
from test_decode_step_gpu import MARGIN, search_case

pytestmark = pytest.mark.gpu
I32 = torch.int32
STEP_BAR = dict(rtol=1e-3, atol=1e-4)
SEEDS = {17: 54, 65: 52, 1: 54}  # float64 margins 3.6e-3, 2.5e-3 and 4.2e-2 (found on the CPU; the test asserts the condition again)


def _spy(monkeypatch, name):
    calls, real = [], getattr(K, name)

    def spy(*a, **k):
        r = real(*a, **k)
        calls.append(r)
        return r

    monkeypatch.setattr(K, name, spy)
    return calls


@pytest.mark.parametrize("B", [17, 65, 1])
def test_transducer_details_against_the_float64_search(dev, monkeypatch, B):
    cfg = configs.conformer_tiny(rnn_units=64, joint_dim=48, vocab_size=40)
    T, d, mode, mtpf = 12, cfg.dmodel, (1 if B == 1 else 0), 3
    W, enc, elen = search_case(SEEDS[B], B, T, d, cfg.embed_dim, 64, 48, 40)
    encj = enc.double() @ W["joint/enc/w"].double() + W["joint/enc/b"].double()
    trace = []
    ref, det = RD.search(mode, W, encj, elen, trace=trace, max_tokens_per_frame=mtpf)
    margin = min(float(m[k].min()) for m, k in trace if k.any())
    present = det["frames"] >= 0
    print(f"smallest top-2 margin {margin:.3e}, {int(present.sum())} symbols")
    assert margin >= MARGIN and present.sum() >= 20
    model = ConformerTransducer(cfg, dev, dtype=torch.float32, seed=0)
    full = model.ps.export_keras()
    full.update(W)
    model.ps.import_keras(full)
    plain = model.recognize_encoded(enc.to(dev), elen, max_tokens_per_frame=mtpf)
    fused_calls, loop_calls = _spy(monkeypatch, "decode_steps_detail"), _spy(monkeypatch, "decode_update_detail")
    out = model.recognize_encoded_detailed(enc.to(dev), elen, max_tokens_per_frame=mtpf)
    torch.cuda.synchronize()
    if B <= 64:  # the fused route ran, and only it
        assert len(fused_calls) > 0 and all(c is True for c in fused_calls) and loop_calls == []
    else:  # B = 65: the per-op loop with the detail bookkeeping kernel
        assert fused_calls == [] and len(loop_calls) > 0
    assert isinstance(out, RecognizeOutput) and out.ends is None and out.vocab_size == 40 and out.seconds_per_frame == model.seconds_per_frame
    # the search itself is untouched
    assert torch.equal(out.predict.tokens, plain.tokens) and torch.equal(out.predict.next_tokens, plain.next_tokens)
    assert torch.equal(out.predict.next_decoder_states, plain.next_decoder_states)
    tokens = out.predict.tokens.cpu().numpy()
    np.testing.assert_array_equal(tokens, ref["tokens"])
    frames, lp, ent = out.frames.cpu().numpy(), out.log_probs.cpu().numpy(), out.entropies.cpu().numpy()
    assert frames.shape == lp.shape == ent.shape == tokens.shape
    np.testing.assert_array_equal(frames, det["frames"])
    np.testing.assert_array_equal(present, tokens != 0 if mode == 1 else (tokens != 0) & (np.arange(tokens.shape[1]) >= 2))
    assert (lp[~present] == 0).all() and (ent[~present] == 0).all()
    np.testing.assert_allclose(lp[present], det["logp"][present], **STEP_BAR)
    np.testing.assert_allclose(ent[present], det["entropy"][present], **STEP_BAR)
    for b in range(B):
        f = frames[b][present[b]]
        assert (np.diff(f) >= 0).all() and (f < elen[b]).all()
        if mode == 1:
            assert np.bincount(f).max() == mtpf  # at most max_tokens_per_frame symbols share a frame, and some frame has that many
    np.testing.assert_allclose(out.scores.cpu().numpy(), np.where(present, lp, 0).sum(1), rtol=1e-5, atol=1e-5)
    conf = token_confidences(out).cpu().numpy()
    np.testing.assert_allclose(conf[present], np.exp(lp[present]), rtol=1e-6)
    assert (conf[~present] == 0).all() and ((token_times(out).cpu().numpy() >= 0) == present).all()


def _ctc_model(dev, seed):
    model = ConformerCTC(configs.conformer_tiny(head="ctc"), dev, dtype=torch.float32, seed=seed)
    with torch.no_grad():
        model.ps.p("dec/logits/w").mul_(3.0)  # peaky frames: tokens among the blanks
    model.ps.refresh_shadow()
    return model


def test_ctc_spans_are_the_forced_alignment_of_the_tokens(dev):
    lens = [8000, 8000, 5000, 6400, 1200]
    rng = np.random.default_rng(5)
    sig = np.clip(rng.standard_normal((len(lens), max(lens))) * 0.1, -1, 1).astype(np.float32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0.0
    inputs = PredictInput(torch.from_numpy(sig), torch.tensor(lens, dtype=I32))
    chosen = None
    for seed in (2, 3, 4, 5, 6, 7):  # the first model whose frames all decide by a clear margin (checked on the host)
        model = _ctc_model(dev, seed)
        logits, elen = model._infer_logits(inputs)
        top = torch.log_softmax(logits.double().cpu(), -1).topk(2, -1).values
        margin = min(float((top[b, :n, 0] - top[b, :n, 1]).min()) for b, n in enumerate(elen) if n > 0)
        print(f"seed {seed}: smallest per-frame top-2 margin {margin:.3e}")
        if margin > 1e-3:
            chosen = seed
            break
    assert chosen is not None
    out = model.recognize_detailed(inputs)
    plain = model.recognize(inputs)
    assert isinstance(out, RecognizeOutput) and torch.equal(out.predict.tokens, plain.tokens)
    tokens = out.predict.tokens.cpu().numpy()
    starts, ends, lp = out.frames.cpu().numpy(), out.ends.cpu().numpy(), out.log_probs.cpu().numpy()
    present = starts >= 0
    tlen = present.sum(1)
    print("tokens per utterance", tlen.tolist(), "frames", [int(v) for v in elen])
    assert tlen.sum() >= 6 and (ends[present] - starts[present]).max() >= 2
    labels = np.where(present, tokens, 0).astype(np.int32)
    preds = np.concatenate([np.zeros((len(lens), 1), np.int32), labels], 1)
    data = TrainData(TrainInput(inputs.inputs, inputs.inputs_length, torch.from_numpy(preds), torch.from_numpy((tlen + 1).astype(np.int32))),
                     TrainLabel(torch.from_numpy(labels), torch.from_numpy(tlen.astype(np.int32))))
    al = model.align(data)
    np.testing.assert_array_equal(al.frames.cpu().numpy(), starts)
    np.testing.assert_array_equal(al.ends.cpu().numpy(), ends)
    n = (ends - starts)[present]
    assert RD.ratio(al.label_log_probs.cpu().numpy()[present], lp[present], n) <= 1.0
    nl = np.asarray([min(int(v), logits.shape[1]) for v in elen])
    assert RD.ratio(al.scores.cpu().numpy()[nl > 0], out.scores.cpu().numpy()[nl > 0], nl[nl > 0]) <= 1.0
    # a token's probability: the geometric mean over its frames
    np.testing.assert_allclose(token_confidences(out).cpu().numpy()[present], np.exp(lp[present] / n), rtol=1e-5)


def test_inherited_classes_return_well_formed_details(dev):
    from tensorflowasr_amd.rnnt import RnnTransducer
    from tensorflowasr_amd.transformer import TransformerCTC

    lens = [6400, 4000, 5200]
    rng = np.random.default_rng(11)
    sig = np.clip(rng.standard_normal((len(lens), max(lens))) * 0.1, -1, 1).astype(np.float32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0.0
    inputs = PredictInput(torch.from_numpy(sig), torch.tensor(lens, dtype=I32))
    for model, ctc in ((RnnTransducer(configs.rnnt_tiny(), dev, dtype=torch.float32, seed=1), False),
                       (TransformerCTC(configs.transformer_tiny(head="ctc"), dev, dtype=torch.float32, seed=1), True)):
        out = model.recognize_detailed(inputs)
        plain = model.recognize(inputs)
        assert isinstance(out, RecognizeOutput) and torch.equal(out.predict.tokens, plain.tokens)
        shape = out.predict.tokens.shape
        assert out.frames.shape == out.log_probs.shape == out.entropies.shape == shape and out.scores.shape == (len(lens),)
        assert out.frames.dtype == I32 and out.log_probs.dtype == out.entropies.dtype == out.scores.dtype == torch.float32
        assert (out.ends is not None) == ctc and out.vocab_size == model.cfg.vocab_size and out.seconds_per_frame == model.seconds_per_frame
        present = (out.frames >= 0).cpu().numpy()
        tokens = out.predict.tokens.cpu().numpy()
        assert ((tokens != model.blank) <= present).all() or ctc  # (a transducer: every symbol has its details)
        if ctc:
            assert (out.ends.cpu().numpy()[present] > out.frames.cpu().numpy()[present]).all() and (tokens[present] != model.blank).all()
        lp, ent = out.log_probs.cpu().numpy(), out.entropies.cpu().numpy()
        assert np.isfinite(lp).all() and np.isfinite(ent).all() and (lp <= 0).all() and (ent >= 0).all()
        assert (ent[present] <= np.log(model.cfg.vocab_size) + 1e-4).all() and (lp[~present] == 0).all()
        conf = token_confidences(out, "entropy").cpu().numpy()
        assert ((conf >= -1e-4) & (conf <= 1)).all()
