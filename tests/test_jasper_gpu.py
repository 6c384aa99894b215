"""JasperCTC (tensorflowasr_amd/jasper.py) on the GPU against the float64 oracle of tests/jasper_oracle.py, and the wiring of the
inherited decoders, alignment, evaluation and checkpoints.

Tiny config: dense, 3 sub-blocks, block channels [64, 96] with kernels [11, 13], first block 48 x 11 stride 2, second block 128, third
block 160, V = 29.  One batch of three utterances of 0.31 s, 0.5 s and 0.8 s.  BatchNorm moving statistics and affine parameters are seeded
non-trivial values.

Whole-depth bf16 error.  It has no bar fixed in advance: the test measures the device's relative error against the f64 oracle, measures
the same for a torch-CPU float64 run of the same layers that rounds the features, the weights and every layer's output to bf16 (the
rounding floor of any bf16 pipeline), allows twice that floor, and writes both numbers to profiles/jasper_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import conformer_ref as R
from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import tokenizers as tk
from tensorflowasr_amd.datasets import ASRSliceDataset
from tensorflowasr_amd.jasper import JasperCTC
from tensorflowasr_amd.schemas import PredictInput, TrainData, TrainInput, TrainLabel

import jasper_oracle as JO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "librispeech", "characters", "english.vocab")
SAMPLES = [4960, 8000, 12800]  # 0.31 s, 0.5 s, 0.8 s
F32_BAR, BF16_BAR = dict(rtol=1e-4, atol=1e-5), dict(rtol=2e-2, atol=2e-2)  # the project's single-layer bars (tests/test_stream_gpu.py)


def tiny_config():
    return configs.jasper_tiny(vocab_size=29, dense=True, nsubblocks=3, block_channels=[64, 96], block_kernels=[11, 13],
                               block_dropout=[0.0, 0.0], first_additional_block_channels=48, first_additional_block_kernels=11,
                               first_additional_block_strides=2, second_additional_block_channels=128, third_additional_block_channels=160)


def build(dev, dtype=torch.float32, seed=3):
    """the initialiser's kernels, seeded non-trivial biases and BatchNorm state (the random shifts keep the signal at O(1) through the
    depth); a decoder that never says ' ' (class 1), so a transcript survives the tokenizer's white-space normalisation unchanged"""
    model = JasperCTC(tiny_config(), dev, dtype=dtype, seed=seed)
    W = model.ps.export_keras()
    g = torch.Generator().manual_seed(100 + seed)
    for name, t in W.items():
        if name.endswith("bn/g"):
            W[name] = torch.rand(t.shape, generator=g) + 0.5
        elif name.endswith("bn/b") or name.endswith("bn/mm"):
            W[name] = torch.randn(t.shape, generator=g) * 0.3
        elif name.endswith("bn/mv"):
            W[name] = torch.rand(t.shape, generator=g) + 0.5
        elif name.endswith("conv1d/b"):
            W[name] = torch.randn(t.shape, generator=g) * 0.1
    W["dec/logits/b"] = W["dec/logits/b"].clone()
    W["dec/logits/b"][1] = -1e4
    model.ps.import_keras(W)
    model.tokenizer = tk.get({"type": "characters", "blank_index": 0, "vocabulary": VOCAB})
    return model


@pytest.fixture(scope="module")
def audio():
    rng = np.random.default_rng(5)
    sig = np.zeros((3, max(SAMPLES)), np.float32)
    for b, n in enumerate(SAMPLES):
        sig[b, :n] = np.clip(rng.standard_normal(n) * 0.1, -1, 1)
    return sig


@pytest.fixture(scope="module")
def model(dev):
    return build(dev)


@pytest.fixture(scope="module")
def reference(model, audio):
    """the f64 oracle of the whole batch, computed once: features, encoder output, logits, the per-layer inputs, and the bf16 floor"""
    c = model.cfg
    W = model.ps.export_keras()
    ocfg = dict(sample_rate=c.sample_rate, frame_ms=c.frame_ms, stride_ms=c.stride_ms, nfft=c.nfft, num_feature_bins=c.num_feature_bins,
                preemphasis=c.preemphasis, epsilon=c.epsilon)
    feats = JO.log10_features(R.log_mel(audio, ocfg))
    trace = []
    enc = JO.encoder(feats, c, W, trace=trace)
    floor = JO.encoder(feats, c, W, rounder=JO.bf16_round, wround=JO.bf16_round)
    flen = [-(-n // c.frame_step) for n in SAMPLES]
    return dict(W=W, feats=feats, enc=enc, logits=JO.logits(enc, W), trace=trace, floor=floor, elen=[c.encoder_length(n) for n in flen])


def _inputs(audio, rows=None):
    rows = range(3) if rows is None else rows
    n = max(SAMPLES[b] for b in rows)
    return PredictInput(torch.from_numpy(audio[list(rows), :n].copy()), torch.tensor([SAMPLES[b] for b in rows], dtype=torch.int32))


def _valid(t, elen):
    return np.concatenate([np.asarray(t[b, :n], np.float64).reshape(n, -1) for b, n in enumerate(elen)])


def _rel(a, b):
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def test_encoder_and_logits_against_the_oracle_f32(model, audio, reference):
    x = _inputs(audio)
    enc, elen = model.encode(x.inputs, x.inputs_length)
    logits, elen2 = model._infer_logits(x)
    torch.cuda.synchronize()
    assert enc.dtype == torch.float32 and list(elen) == list(elen2) == reference["elen"] == [16, 25, 40]
    np.testing.assert_allclose(_valid(enc.cpu(), elen), _valid(reference["enc"], elen), **F32_BAR)
    np.testing.assert_allclose(_valid(logits.cpu(), elen), _valid(reference["logits"], elen), **F32_BAR)
    out = model(TrainInput(x.inputs, x.inputs_length, None, None))
    assert out.logits.shape == (3, 40, 29) and out.logits_length.tolist() == [16, 25, 40]


def test_bf16_layer_by_layer_and_whole_depth(dev, audio, reference):
    m16 = build(dev, torch.bfloat16)
    for li, (mod, (x, residuals)) in enumerate(zip(m16.layers, reference["trace"])):
        xd = x.to(torch.bfloat16).to(dev).contiguous()
        rd = [r.to(torch.bfloat16).to(dev).contiguous() for r in residuals]
        y = m16._layer_fwd(xd, mod, rd)
        # the oracle sees the same bf16-rounded input and weights
        omod = JO.topology(m16.cfg)[li]
        assert omod["name"] == mod["name"]
        ref = JO.layer(JO.bf16_round(x), omod, [JO.bf16_round(r) for r in residuals], reference["W"], wround=JO.bf16_round)
        np.testing.assert_allclose(y.float().cpu().numpy(), ref.numpy(), **BF16_BAR, err_msg=mod["name"])
    x = _inputs(audio)
    enc, elen = m16.encode(x.inputs, x.inputs_length, precision="bf16")
    torch.cuda.synchronize()
    assert enc.dtype == torch.bfloat16
    want = _valid(reference["enc"], elen)
    err, floor = _rel(_valid(enc.float().cpu(), elen), want), _rel(_valid(reference["floor"], elen), want)
    print(f"whole-depth bf16 relative error {err:.3e}, rounding floor {floor:.3e}")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "jasper_parity.json"), "w") as f:
        json.dump({"config": "tiny (tests/test_jasper_gpu.py)", "bf16_whole_depth_rel_error": err, "bf16_rounding_floor": floor,
                   "allowed": 2 * floor}, f, indent=1)
        f.write("\n")
    assert floor > 0 and err <= 2 * floor
    # the default precision of a bf16 model is the f32 twin on the same weights
    e32, _ = m16.encode(x.inputs, x.inputs_length)
    assert e32.dtype == torch.float32
    np.testing.assert_allclose(_valid(e32.cpu(), elen), want, **F32_BAR)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_batch_row_equals_the_utterance_alone(dev, model, audio, dtype):
    """Valid frames of a batch row are bit-equal to the utterance encoded alone.  Two forms.  (a) `encode` of the row alone, in a buffer
    that keeps (some of) the zero padding a batch puts behind it: the front end pre-emphasises the padded signal as the reference does
    (feature_extraction.py: s[n] - 0.97 s[n-1] over the whole row), so the first padding sample is -0.97 times the last real one, which
    a buffer cut at the utterance's last sample does not hold - a property of the shared front end, not of this encoder.  (b) the encoder
    alone on the row's features cut at the utterance's own length, so T differs (31 / 50 against 80 frames) and nothing lies behind."""
    m = model if dtype == torch.float32 else build(dev, dtype)
    prec = "f32" if dtype == torch.float32 else "bf16"
    em = m  # (precision names the model's own type: no twin is involved)
    x = _inputs(audio)
    enc, elen = m.encode(x.inputs, x.inputs_length, precision=prec)
    feats, flen = em.frontend(x.inputs.to(dev), [int(v) for v in x.inputs_length])
    for b in range(3):
        n = min(SAMPLES[b] + 160, audio.shape[1])
        one = PredictInput(torch.from_numpy(audio[b:b + 1, :n].copy()), torch.tensor([SAMPLES[b]], dtype=torch.int32))
        e1, l1 = m.encode(one.inputs, one.inputs_length, precision=prec)
        assert l1 == [elen[b]] and torch.equal(e1[0, :l1[0]], enc[b, :elen[b]]), b
        # against the buffer cut at the last sample only the frames that see the boundary sample may differ: feature frames from
        # (n - frame_length) // step + 1 on hold sample n, and encoder frame t reads feature frames <= 2 t through causal layers only
        cut = PredictInput(torch.from_numpy(audio[b:b + 1, :SAMPLES[b]].copy()), torch.tensor([SAMPLES[b]], dtype=torch.int32))
        e0, _ = m.encode(cut.inputs, cut.inputs_length, precision=prec)
        first_feat = max((SAMPLES[b] - m.cfg.frame_length) // m.cfg.frame_step + 1, 0)
        clean = first_feat // 2 + (first_feat % 2)  # encoder frames t with 2 t < first_feat
        assert torch.equal(e0[0, :clean], enc[b, :clean]), b
        e2, T2, l2, _ = em.encoder_fwd(feats[b:b + 1, :flen[b]].contiguous(), [flen[b]], False, None)
        assert l2 == [elen[b]] and T2 == elen[b] and torch.equal(e2.view(T2, -1), enc[b, :elen[b]]), b


def _collapse(logits, n, blank=0):
    path = np.argmax(np.asarray(logits[:n]), -1)
    keep = [int(c) for k, c in enumerate(path) if c != blank and (k == 0 or c != path[k - 1])]
    return keep


def test_decoders_are_wired(model, audio):
    x = _inputs(audio)
    logits, elen = model._infer_logits(x)
    host = logits.cpu().numpy()
    greedy = model.recognize(x).tokens.cpu().numpy()
    want = [_collapse(host[b], elen[b]) for b in range(3)]
    assert all(len(w) > 3 for w in want)  # the model speaks
    for b in range(3):
        assert [int(v) for v in greedy[b] if v != 0] == want[b]
    bh = model.recognize_beam(x, beam_width=4).tokens.cpu().numpy()
    bd = model.recognize_beam(x, beam_width=4, device_search=True).tokens.cpu().numpy()
    nb, nlen, _ = model.recognize_nbest(x, beam_width=4, top_paths=2)
    nb, nlen = nb.cpu().numpy(), nlen.cpu().numpy()
    for b in range(3):
        first = [int(v) for v in nb[b, 0, :nlen[b, 0]]]
        strip = lambda row: [int(v) for v in row[:len(first)]]
        assert strip(bh[b]) == first and strip(bd[b]) == first and not bh[b, len(first):].any() and not bd[b, len(first):].any(), b


def test_align_and_evaluate(model, audio, tmp_path):
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
    # a two-utterance .tsv whose transcripts are the model's own: zero errors at every level
    texts = model.tokenizer.detokenize(greedy.numpy())
    wav = {f"utt{b}.wav": audio[b, :SAMPLES[b]] for b in (1, 2)}
    tsv = os.path.join(tmp_path, "own.tsv")
    with open(tsv, "w", encoding="utf-8") as f:
        f.write("PATH\tDURATION\tTRANSCRIPT\n")
        for b in (1, 2):
            assert len(texts[b].strip()) > 3
            f.write(f"utt{b}.wav\t{SAMPLES[b] / 16000:.2f}\t{texts[b]}\n")
    ds = ASRSliceDataset("test", model.tokenizer, [tsv], reader=lambda path, sr: wav[os.path.basename(path)])
    rows = model.evaluate(ds, batch_size=2)
    g = rows["greedy"]
    assert g["utterances"] == 2 and g["wer"] == 0 and g["cer"] == 0 and g["ter"] == 0
    assert g["tokens"]["distance"] == 0 and g["tokens"]["ref_length"] == int(llen[1] + llen[2])


def test_npz_round_trip_into_another_seed(dev, model, audio, tmp_path):
    path = os.path.join(tmp_path, "jasper.npz")
    names = model.save_weights(path)
    assert "encoder/block_1/subordinate_2/residual_1/pointwise_conv1d/kernel" in names and "decoder/logits/kernel" in names
    with np.load(path) as z:
        assert z["decoder|logits|kernel"].shape == (1, 160, 29) and z["encoder|first_block|conv1d|kernel"].shape == (11, 80, 48)
    other = JasperCTC(tiny_config(), dev, dtype=torch.float32, seed=11)
    x = _inputs(audio)
    before, _ = other._infer_logits(x)
    want, _ = model._infer_logits(x)
    assert not torch.equal(before, want)
    other.load_weights(path)  # (the folded BatchNorm pairs made for `before` must not survive the load)
    got, _ = other._infer_logits(x)
    assert torch.equal(got, want)
    with pytest.raises(NotImplementedError):
        model.save_weights(os.path.join(tmp_path, "jasper.weights.h5"))


def test_training_is_refused(model, audio):
    x = _inputs(audio)
    data = TrainData(TrainInput(x.inputs, x.inputs_length, None, None), TrainLabel(torch.ones(3, 2, dtype=torch.int32), torch.tensor([2, 2, 2])))
    for call in (lambda: model.train_step(data), lambda: model.loss_and_backward(data), lambda: model.compile()):
        with pytest.raises(NotImplementedError, match="inference only"):
            call()
    with pytest.raises(ValueError):
        JasperCTC(configs.conformer_tiny(head="ctc"), model.device)
