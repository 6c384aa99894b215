"""DeepSpeech2CTC (tensorflowasr_amd/deepspeech2.py) on the GPU against the float64 oracle of tests/ds2_oracle.py, and the wiring of the
inherited decoders, alignment, evaluation and checkpoints.

Tiny configs, V = 29, F = 16 spectrogram bins, one batch of three utterances of 0.31 s, 0.5 s and 0.8 s:
  bidirectional  conv (5,7)/(2,2) -> 16 and (3,5)/(1,2) -> 16 "same", 2 x BiLSTM(32), 1 x FC(64)
  unidirectional the same convolutions causal, 2 x LSTM(32) each followed by RowConv1D(2), 1 x FC(64)
BatchNorm moving statistics and affine parameters are seeded non-trivial values (ds2_cases.make_weights).

f32 bars.  Per layer (the device layer on the oracle's input of that layer): the project's single-layer bar, rtol 1e-4 / atol 1e-5.  At
whole depth the bar is that times the number of layers in the chain (2 conv + 2 RNN blocks + 1 FC, + 1 for the logits; the front end's
own 2e-5 is inside the first share): every layer adds at most its own bar to what it passes on, and none of these layers amplifies
(BatchNorm scales are <= 1.5 / sqrt(0.5), the LSTM's outputs are bounded gates times tanh, the kernels are Glorot-scaled).

Whole-depth bf16 error.  It has no bar fixed in advance: the test measures the device's relative error against the f64 oracle, measures
the same for a torch-CPU float64 run of the same layers that rounds the features, the weights and every layer's output to bf16 (the
rounding floor of any bf16 pipeline), allows twice that floor, and writes both numbers to profiles/deepspeech2_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import tokenizers as tk
from tensorflowasr_amd.datasets import ASRSliceDataset
from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC
from tensorflowasr_amd.schemas import PredictInput, TrainData, TrainInput, TrainLabel

import ds2_cases as C
import ds2_oracle as DO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "librispeech", "characters", "english.vocab")
SAMPLES = C.SAMPLES
F32_BAR, BF16_BAR = dict(rtol=1e-4, atol=1e-5), dict(rtol=2e-2, atol=2e-2)  # the project's single-layer bars (tests/test_jasper_gpu.py)
FEAT_BAR = dict(rtol=0, atol=2e-5)  # the log-mel front end's bar (tests/test_ops_gpu.py::test_logmel)


def _depth_bar(cfg):
    n = len(cfg.conv_filters) + cfg.rnn_nlayers + cfg.fc_nlayers + 1
    return dict(rtol=n * F32_BAR["rtol"], atol=n * F32_BAR["atol"])


def build(dev, variant="bi", dtype=torch.float32):
    cfg = C.tiny_config(variant)
    model = DeepSpeech2CTC(cfg, dev, dtype=dtype, seed=C.SEED[variant])
    model.ps.import_keras(C.make_weights(cfg))
    model.tokenizer = tk.get({"type": "characters", "blank_index": 0, "vocabulary": VOCAB})
    return model


@pytest.fixture(scope="module")
def audio():
    return C.audio()


@pytest.fixture(scope="module")
def models(dev):
    return {v: build(dev, v) for v in ("bi", "uni")}


@pytest.fixture(scope="module")
def references(audio):
    """the f64 oracle of the whole batch per variant, computed once on the CPU (tests/ds2_cases.py)"""
    return {v: C.reference(v, audio) for v in ("bi", "uni")}


def _inputs(audio, rows=None):
    rows = range(3) if rows is None else rows
    n = max(SAMPLES[b] for b in rows)
    return PredictInput(torch.from_numpy(audio[list(rows), :n].copy()), torch.tensor([SAMPLES[b] for b in rows], dtype=torch.int32))


def _valid(t, elen):
    return np.concatenate([np.asarray(t[b, :n], np.float64).reshape(n, -1) for b, n in enumerate(elen)])


def _rel(a, b):
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


@pytest.mark.parametrize("F", [16, 160])
def test_spectrogram_features(dev, audio, F):
    cfg = C.tiny_config("bi", num_feature_bins=F, conv_kernels=[[5, 7], [3, 5]])
    m = DeepSpeech2CTC(cfg, dev, dtype=torch.float32, seed=1)
    x = _inputs(audio)
    feats, flen = m.frontend(x.inputs.to(dev), [int(v) for v in x.inputs_length])
    assert feats.shape == (3, 80, F) and flen == [31, 50, 80]
    np.testing.assert_allclose(feats.cpu().numpy(), DO.spectrogram(audio, cfg).numpy(), **FEAT_BAR)


@pytest.mark.parametrize("variant", ["bi", "uni"])
def test_layers_encoder_and_logits_against_the_oracle_f32(dev, models, references, audio, variant):
    model, ref = models[variant], references[variant]
    cfg, tr = model.cfg, ref["trace"]
    lens_dev = torch.tensor(ref["elen"], dtype=torch.int32, device=dev)
    # layer by layer on the oracle's inputs
    for m in model.modules["convs"]:
        w, bias, scale, shift = model._conv_consts(m["name"])
        y = K.conv2d_fwd(tr[m["name"]].float().to(dev).contiguous(), w, (m["kh"], m["kw"], m["cin"], m["cout"]), bias=bias, scale=scale,
                         shift=shift, relu=True, strides=(m["st"], m["sf"]), padding=cfg.conv_padding)
        want = DO.conv_block(tr[m["name"]].float(), m["name"], (m["st"], m["sf"]), cfg, ref["W"])
        np.testing.assert_allclose(y.cpu().numpy(), want.numpy(), **F32_BAR, err_msg=m["name"])
    _, otopo, _ = DO.topology(cfg)
    for r, o in zip(model.modules["rnns"], otopo):
        x = tr[r["name"]].float()
        y = model.rnn_block_fwd(x.to(dev).contiguous(), r, lens_dev)
        want = DO.rnn_block(x, o, ref["elen"], ref["W"])
        np.testing.assert_allclose(y.cpu().numpy(), want.numpy(), **F32_BAR, err_msg=r["name"])
        yl = model.lstm_fwd(x.to(dev).contiguous(), r, lens_dev)
        for b, n in enumerate(ref["elen"]):  # frames at or past the reduced length leave every LSTM as exact zeros
            assert not yl[b, n:].any() and (n == 0 or yl[b, :n].any()), (r["name"], b)
    # whole depth
    x = _inputs(audio)
    enc, elen = model.encode(x.inputs, x.inputs_length)
    logits, elen2 = model._infer_logits(x)
    torch.cuda.synchronize()
    assert enc.dtype == torch.float32 and list(elen) == list(elen2) == ref["elen"] == [16, 25, 40]
    bar = _depth_bar(cfg)
    np.testing.assert_allclose(_valid(enc.cpu(), elen), _valid(ref["enc"], elen), **bar)
    np.testing.assert_allclose(_valid(logits.cpu(), elen), _valid(ref["logits"], elen), **bar)
    out = model(TrainInput(x.inputs, x.inputs_length, None, None))
    assert out.logits.shape == (3, 40, 29) and out.logits_length.tolist() == [16, 25, 40]


@pytest.mark.parametrize("variant", ["bi", "uni"])
def test_greedy_tokens_equal_the_oracles(models, references, audio, variant):
    model, ref = models[variant], references[variant]
    assert ref["margin"] > 1e-3  # a condition on the input (tests/test_ds2_oracle.py checks it on the CPU): no near-tied frame
    greedy = model.recognize(_inputs(audio)).tokens.cpu().numpy()
    assert all(len(w) > 3 for w in ref["tokens"])  # the model speaks
    for b in range(3):
        assert [int(v) for v in greedy[b] if v != 0] == ref["tokens"][b], b


@pytest.mark.parametrize("variant", ["bi", "uni"])
def test_bf16_whole_depth(dev, references, audio, variant):
    ref = references[variant]
    m16 = build(dev, variant, torch.bfloat16)
    x = _inputs(audio)
    enc, elen = m16.encode(x.inputs, x.inputs_length, precision="bf16")
    torch.cuda.synchronize()
    assert enc.dtype == torch.bfloat16
    want = _valid(ref["enc"], elen)
    err, floor = _rel(_valid(enc.float().cpu(), elen), want), _rel(_valid(ref["floor"], elen), want)
    print(f"{variant}: whole-depth bf16 relative error {err:.3e}, rounding floor {floor:.3e}")
    path = os.path.join(ROOT, "profiles", "deepspeech2_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    rec = {}
    if os.path.exists(path):
        with open(path) as f:
            rec = json.load(f)
    rec[variant] = {"config": f"tiny {variant} (tests/test_ds2_gpu.py)", "bf16_whole_depth_rel_error": err, "bf16_rounding_floor": floor,
                    "allowed": 2 * floor}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    assert floor > 0 and err <= 2 * floor
    # the default precision of a bf16 model is the f32 twin on the same weights
    e32, _ = m16.encode(x.inputs, x.inputs_length)
    assert e32.dtype == torch.float32
    np.testing.assert_allclose(_valid(e32.cpu(), elen), want, **_depth_bar(m16.cfg))


def test_unidirectional_causal_row_equals_the_utterance_alone(dev, models, audio):
    """causal convolutions, forward LSTMs and a causal RowConv1D: frame t depends on frames <= t only, so what lies behind an utterance's
    end in its batch row cannot reach a valid frame.  The encoder alone on the row's features cut at the utterance's own length (T = 31 /
    50 against 80 frames, nothing behind) gives the batch's valid frames at the f32 bar."""
    m = models["uni"]
    x = _inputs(audio)
    enc, elen = m.encode(x.inputs, x.inputs_length)
    feats, flen = m.frontend(x.inputs.to(dev), [int(v) for v in x.inputs_length])
    for b in range(3):
        e2, T2, l2, _ = m.encoder_fwd(feats[b:b + 1, :flen[b]].contiguous(), [flen[b]], False, None)
        assert l2 == [elen[b]] and T2 == elen[b]
        np.testing.assert_allclose(e2.view(T2, -1).cpu().numpy(), enc[b, :elen[b]].cpu().numpy(), **F32_BAR)


def test_bidirectional_same_row_is_not_the_utterance_alone(dev, models, audio):
    """the reference's behaviour on a padded batch, reproduced: with "same" padding the last valid frames of a short utterance see the
    padded tail's features (ln(eps), not 0), so row 0 of the batch differs from utterance 0 run alone - while the longest row does not"""
    m = models["bi"]
    x = _inputs(audio)
    enc, elen = m.encode(x.inputs, x.inputs_length)
    feats, flen = m.frontend(x.inputs.to(dev), [int(v) for v in x.inputs_length])
    e0, T0, _, _ = m.encoder_fwd(feats[0:1, :flen[0]].contiguous(), [flen[0]], False, None)
    assert not np.allclose(e0.view(T0, -1).cpu().numpy(), enc[0, :elen[0]].cpu().numpy(), **F32_BAR)
    e2, T2, _, _ = m.encoder_fwd(feats[2:3].contiguous(), [flen[2]], False, None)
    np.testing.assert_allclose(e2.view(T2, -1).cpu().numpy(), enc[2].cpu().numpy(), **F32_BAR)


def test_decoders_are_wired(models, references, audio):
    model, ref = models["bi"], references["bi"]
    x = _inputs(audio)
    bh = model.recognize_beam(x, beam_width=4).tokens.cpu().numpy()
    bd = model.recognize_beam(x, beam_width=4, device_search=True).tokens.cpu().numpy()
    nb, nlen, _ = model.recognize_nbest(x, beam_width=4, top_paths=2)
    nb, nlen = nb.cpu().numpy(), nlen.cpu().numpy()
    for b in range(3):
        first = [int(v) for v in nb[b, 0, :nlen[b, 0]]]
        strip = lambda row: [int(v) for v in row[:len(first)]]
        assert strip(bh[b]) == first and strip(bd[b]) == first and not bh[b, len(first):].any() and not bd[b, len(first):].any(), b
        assert nlen[b, 1] > 0 and [int(v) for v in nb[b, 1, :nlen[b, 1]]] != first


def test_align_and_evaluate(models, audio, tmp_path):
    model = models["bi"]
    x = _inputs(audio)
    _, elen = model._infer_logits(x)
    greedy = model.recognize(x).tokens.cpu()
    llen = (greedy != 0).sum(1).to(torch.int32)
    labels = torch.zeros_like(greedy)
    for b in range(3):
        labels[b, :llen[b]] = greedy[b][greedy[b] != 0]
    out = model.align(TrainData(TrainInput(x.inputs, x.inputs_length, None, None), TrainLabel(labels, llen)))
    start, end, score = out.frames.cpu().numpy(), out.ends.cpu().numpy(), out.scores.cpu().numpy()
    assert np.isfinite(score).all()
    for b in range(3):
        n = int(llen[b])
        assert (start[b, :n] >= 0).all() and (end[b, :n] <= elen[b]).all() and (start[b, :n] < end[b, :n]).all(), b
    # a two-utterance .tsv whose transcripts are the model's own: zero errors at every level, and the results file is written
    texts = model.tokenizer.detokenize(greedy.numpy())
    wav = {f"utt{b}.wav": audio[b, :SAMPLES[b]] for b in (1, 2)}
    tsv = os.path.join(tmp_path, "own.tsv")
    with open(tsv, "w", encoding="utf-8") as f:
        f.write("PATH\tDURATION\tTRANSCRIPT\n")
        for b in (1, 2):
            assert len(texts[b].strip()) > 3
            f.write(f"utt{b}.wav\t{SAMPLES[b] / 16000:.2f}\t{texts[b]}\n")
    ds = ASRSliceDataset("test", model.tokenizer, [tsv], reader=lambda path, sr: wav[os.path.basename(path)])
    result = os.path.join(tmp_path, "result.tsv")
    rows = model.evaluate(ds, output_file_path=result, batch_size=2)
    g = rows["greedy"]
    assert g["utterances"] == 2 and g["wer"] == 0 and g["cer"] == 0 and g["ter"] == 0
    assert g["tokens"]["distance"] == 0 and g["tokens"]["ref_length"] == int(llen[1] + llen[2])
    with open(result, encoding="utf-8") as f:
        lines = f.read().splitlines()
    assert len(lines) == 3 and lines[0].split("\t")[:3] == ["PATH", "GROUND_TRUTH", "GREEDY"] and texts[1].strip() in lines[1]


def test_npz_round_trip_into_another_seed(dev, models, audio, tmp_path):
    for variant, must in (("bi", "encoder/rnn_module/block_1/blstm/backward_lstm/recurrent_kernel"),
                          ("uni", "encoder/rnn_module/block_0/rowconv/conv/kernel")):
        model = models[variant]
        path = os.path.join(tmp_path, f"ds2_{variant}.npz")
        names = model.save_weights(path)
        assert must in names and "decoder/logits/kernel" in names and "encoder/conv_module/block_0/bn/moving_variance" in names
        with np.load(path) as z:
            assert z["decoder|logits|kernel"].shape == (64, 29) and z["encoder|conv_module|block_0|conv2d|kernel"].shape == (5, 7, 1, 16)
            if variant == "uni":
                assert z["encoder|rnn_module|block_0|rowconv|conv|kernel"].shape == (5, 32, 1)
        other = DeepSpeech2CTC(C.tiny_config(variant), dev, dtype=torch.float32, seed=11)
        x = _inputs(audio)
        before, _ = other._infer_logits(x)
        want, _ = model._infer_logits(x)
        assert not torch.equal(before, want)
        other.load_weights(path)  # (the folded BatchNorm pairs and concatenated kernels made for `before` must not survive the load)
        got, _ = other._infer_logits(x)
        assert torch.equal(got, want)
    with pytest.raises(NotImplementedError):
        models["bi"].save_weights(os.path.join(tmp_path, "ds2.weights.h5"))


def test_training_and_streaming_are_refused(models, audio):
    model = models["bi"]
    x = _inputs(audio)
    data = TrainData(TrainInput(x.inputs, x.inputs_length, None, None), TrainLabel(torch.ones(3, 2, dtype=torch.int32), torch.tensor([2, 2, 2])))
    for call in (lambda: model.train_step(data), lambda: model.loss_and_backward(data), lambda: model.compile(), lambda: model.stream(),
                 lambda: model.stream_state(), lambda: model.encode_chunk(None, None, None)):
        with pytest.raises(NotImplementedError, match="inference only"):
            call()
    with pytest.raises(ValueError):
        DeepSpeech2CTC(configs.conformer_tiny(head="ctc"), model.device)
