"""recognize_beam_lm / recognize_nbest_lm on a tiny model of each CTC class (random weights) equal the host fused routine run on that
model's own logits; evaluate(lm=...) scores what recognize_beam_lm returns, evaluate without lm is unchanged, and a transducer
refuses lm=."""
import numpy as np
import pytest
import torch

import ctc_lm_oracle as O
import test_evaluate_gpu as EV
from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.schemas import PredictInput

pytestmark = pytest.mark.gpu
ALPHA, BETA = 0.8, 0.3


def _model(kind, dev):
    from tensorflowasr_amd.ctc_model import ConformerCTC
    from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC
    from tensorflowasr_amd.jasper import JasperCTC
    from tensorflowasr_amd.transformer import TransformerCTC

    if kind == "conformer":
        return ConformerCTC(configs.conformer_tiny(head="ctc", vocab_size=29), dev, dtype=torch.float32, seed=3)
    if kind == "transformer":
        return TransformerCTC(configs.transformer_tiny(), dev, dtype=torch.float32, seed=1)
    if kind == "jasper":
        return JasperCTC(configs.jasper_tiny(), dev, dtype=torch.float32, seed=1)
    return DeepSpeech2CTC(configs.deepspeech2_tiny(), dev, dtype=torch.float32, seed=1)


@pytest.mark.parametrize("kind", ["conformer", "transformer", "jasper", "deepspeech2"])
def test_model_methods_equal_the_host_routine_on_the_models_logits(dev, kind):
    model = _model(kind, dev)
    with torch.no_grad():  # peaky outputs, so that the hypotheses are not all empty
        model.ps.p("dec/logits/w").mul_(3.0)
    model.ps.refresh_shadow()
    lens = [6400, 4000, 5200]
    rng = np.random.default_rng(11)
    sig = np.clip(rng.standard_normal((len(lens), max(lens))) * 0.1, -1, 1).astype(np.float32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0.0
    inputs = PredictInput(torch.from_numpy(sig), torch.tensor(lens, dtype=torch.int32))
    V, blank = model.cfg.vocab_size, int(model.blank)
    lm = O.markov_lm(V, blank, 3, seed=5)
    logits, elen = model._infer_logits(inputs)
    W, P = 4, 3
    ht, hn, hs, hlp, hls = K.ctc_beam_search_lm_host(logits, torch.tensor(elen, dtype=torch.int32), lm.tables(ALPHA, BETA), beam_width=W,
                                                     top_paths=P, blank_index=blank)
    toks, n, score, lp, ls = (t.cpu() for t in model.recognize_nbest_lm(inputs, lm, beam_width=W, top_paths=P, alpha=ALPHA, beta=BETA))
    assert torch.equal(toks, ht) and torch.equal(n, hn) and torch.equal(ls, hls)
    np.testing.assert_allclose(lp.numpy(), hlp.numpy(), rtol=0, atol=1e-4)
    assert torch.equal(score, lp + ls)
    assert int(hn[:, 0].sum()) > 0
    width = max(int(hn[:, 0].max()), 1)
    top = model.recognize_beam_lm(inputs, lm, beam_width=W, alpha=ALPHA, beta=BETA)
    assert top.tokens.is_cuda and torch.equal(top.tokens.cpu(), ht[:, 0, :width])
    onhost = model.recognize_beam_lm(inputs, lm, beam_width=W, alpha=ALPHA, beta=BETA, device_search=False)
    assert torch.equal(onhost.tokens.cpu(), ht[:, 0, :width])
    with pytest.raises(ValueError, match="32"):
        model.recognize_beam_lm(inputs, lm, beam_width=33)


def test_evaluate_with_an_lm_scores_recognize_beam_lm(dev, tmp_path):
    model = EV.build("ctc", dev)
    tok, blank = model.tokenizer, int(model.blank)
    ds = EV.make_dataset(tok, str(tmp_path))
    lm = O.markov_lm(tok.num_classes, blank, 3, seed=5)
    data = list(EV.batches(ds, dev))
    plain = model.evaluate(data, beam_width=4, top_paths=2)
    fused = model.evaluate(data, beam_width=4, top_paths=2, lm=lm, lm_alpha=ALPHA, lm_beta=BETA)
    again = model.evaluate(data, beam_width=4, top_paths=2)
    assert repr(plain) == repr(again)  # (repr: nan != nan)
    assert repr(fused["greedy"]) == repr(plain["greedy"])
    beam, labels = [], []
    for x, y in data:
        inp = EV.predict_input(model, x)
        beam.append(model.recognize_beam_lm(inp, lm, beam_width=4, alpha=ALPHA, beta=BETA).tokens.cpu().numpy())
        labels.append((y.labels.cpu().numpy().astype(np.int32), y.labels_length.cpu().numpy().astype(np.int32)))
    stats, _, _ = EV.host_row(beam, labels, tok, blank)
    EV.same_row(fused["beam"], stats, len(EV.TEXTS))
    assert set(fused) == {"greedy", "beam", "oracle"} and fused["oracle"]["utterances"] == len(EV.TEXTS)


def test_a_transducer_refuses_an_lm(dev, tmp_path):
    model = EV.build("conformer", dev)
    ds = EV.make_dataset(model.tokenizer, str(tmp_path))
    lm = O.markov_lm(model.tokenizer.num_classes, int(model.blank), 2, seed=5)
    with pytest.raises(NotImplementedError, match="CTC"):
        model.evaluate(list(EV.batches(ds, dev)), beam_width=4, lm=lm)
