"""TransformerCTC / TransformerTransducer (tensorflowasr_amd/transformer.py) on the GPU against the float64 oracle of
tests/transformer_oracle.py and the recorded run of the reference's own classes (tests/golden/transformer_wiring.npz), and the wiring of
the inherited decoders, alignment, evaluation and checkpoints.

Tiny model (tests/transformer_cases.py): F = 16 mel bins, 16 filters, d = 64, 2 heads of 64, dff = 128, 2 blocks, V = 29; one batch of three
utterances of 0.31 s, 0.5 s and 0.8 s (8 / 13 / 20 encoder frames); "full" attention and "chunked" (chunk 4, history 8).

f32 bars.  Against the f64 oracle, on the SAME operands (the oracle's features, or the oracle's input of a block): the largest absolute
error of the oracle's own arithmetic run in float32 by torch on the CPU, times 4 for the summation order.  Against the recorded reference
run the fixture's own distance from the f64 oracle is added (it is a run that stores float32 between layers).  Whole-depth bf16: the
DeepSpeech2 test's method - the relative error against the f64 oracle may be twice the rounding floor, a float64 CPU run that rounds the
features, the weights, every stored activation and the probabilities before P V to bf16.  All figures go to profiles/transformer_parity.json.
Every row is compared, padded ones included: they are live (their keys feed the next block)."""
import json
import os

import numpy as np
import pytest
import torch

from tensorflowasr_amd import base_model, configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import tokenizers as tk
from tensorflowasr_amd.datasets import ASRSliceDataset
from tensorflowasr_amd.schemas import PredictInput, TrainData, TrainInput, TrainLabel
from tensorflowasr_amd.transformer import TransformerCTC, TransformerTransducer

import transformer_cases as C
import transformer_oracle as TO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "librispeech", "characters", "english.vocab")
PARITY = os.path.join(ROOT, "profiles", "transformer_parity.json")
SAMPLES = C.SAMPLES
VARIANTS = {"full": ("full", {}), "chunked": ("chunked", {}),
            "pre": ("full", dict(norm_position="pre", residual_factor=0.5, interleave_relpe=False)),
            "causal": ("chunked", dict(use_attention_causal_mask=True, sub_norm="none")), "nomask": ("full", dict(use_attention_auto_mask=False)),
            "dh128": ("full", dict(head_size=128))}


def _record(key, **figures):
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    rec = {}
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            rec = json.load(f)
    rec.setdefault(key, {}).update(figures)
    with open(PARITY, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def build(dev, variant="full", dtype=torch.float32, cls=TransformerCTC, head="ctc"):
    setting, over = VARIANTS[variant]
    cfg = C.tiny_config(setting, head=head, **over)
    model = cls(cfg, dev, dtype=dtype, seed=3)
    model.ps.import_keras(C.make_weights(cfg))
    model.tokenizer = tk.get({"type": "characters", "blank_index": 0, "vocabulary": VOCAB})
    return model


@pytest.fixture(scope="module")
def audio():
    return C.audio()


@pytest.fixture(scope="module")
def models(dev):
    return {v: build(dev, v) for v in ("full", "chunked")}


_REFS = {}


def reference(variant):
    """the f64 / f32 / bf16-rounded oracle runs of one variant, computed once on the CPU"""
    if variant not in _REFS:
        setting, over = VARIANTS[variant]
        _REFS[variant] = C.reference(setting, cfg=C.tiny_config(setting, **over))
    return _REFS[variant]


def _inputs(audio, rows=None):
    rows = range(3) if rows is None else rows
    n = max(SAMPLES[b] for b in rows)
    return PredictInput(torch.from_numpy(audio[list(rows), :n].copy()), torch.tensor([SAMPLES[b] for b in rows], dtype=torch.int32))


def _maxerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def _encode(model, ref, dev):
    """the encoder on the ORACLE's features (the same operands), every row"""
    feats = ref["feats"].to(model.dtype).to(dev).contiguous()
    x, T, lens, _ = model.encoder_fwd(feats, ref["flen"], False, None)
    torch.cuda.synchronize()
    assert lens == ref["elen"] == C.ELEN and T == 20
    return x.view(3, T, -1)


@pytest.mark.parametrize("setting", ["full", "chunked"])
def test_load_weights_of_the_wiring_fixture_reproduces_the_recorded_run(dev, setting, tmp_path):
    with np.load(C.WIRING) as z:
        wiring = {k: z[k] for k in z.files}
    path = os.path.join(tmp_path, "wiring.npz")
    with open(path, "wb") as f:  # the fixture's weights as a checkpoint file under the reference's names
        np.savez(f, **{k[2:]: v for k, v in wiring.items() if k.startswith("w|")})
    model = TransformerCTC(C.tiny_config(setting), dev, dtype=torch.float32, seed=99)
    names = model.load_weights(path)
    assert "enc/block_1/mhsa/k/w" in names and len(names) == 48
    ref = reference(setting)
    assert np.array_equal(wiring["feats"], ref["feats"].float().numpy())
    enc = _encode(model, ref, dev)
    logits = K.matmul(enc.reshape(60, 64), model.ps.p2d("dec/logits/w"), bias=model.ps.p("dec/logits/b")).view(3, 20, 29)
    want_e, want_l = wiring[f"{setting}|encoder"], wiring[f"{setting}|logits"]
    e_bar = 4 * _maxerr(ref["enc32"], ref["enc"]) + _maxerr(want_e, ref["enc"])
    l_bar = 4 * _maxerr(ref["logits32"], ref["logits"]) + _maxerr(want_l, ref["logits"])
    e_err, l_err = _maxerr(enc.cpu(), want_e), _maxerr(logits.cpu(), want_l)
    print(f"{setting}: against the recorded reference run: encoder {e_err:.3e} (bar {e_bar:.3e}), logits {l_err:.3e} (bar {l_bar:.3e})")
    _record(f"wiring_{setting}", encoder_error=e_err, encoder_bar=e_bar, logits_error=l_err, logits_bar=l_bar)
    assert e_err <= e_bar and l_err <= l_bar


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_blocks_and_whole_depth_against_the_oracle_f32(dev, variant):
    model, ref = build(dev, variant), reference(variant)
    cfg, W = ref["cfg"], ref["W"]
    lens_dev = torch.tensor(ref["elen"], dtype=torch.int32, device=dev)
    # subsampling + linear + masked position table on the oracle's features
    x, T, lens, _ = model.embed_fwd(ref["feats"].float().to(dev).contiguous(), ref["flen"])
    want = ref["trace"]["enc/block_0"]
    bar = 4 * _maxerr(TO.embed(ref["feats"], ref["flen"], cfg, W, torch.float32)[0], want)
    err = _maxerr(x.view(3, T, -1).cpu(), want)
    figures = {"embed_error": err, "embed_bar": bar}
    assert err <= bar, ("embed", err, bar)
    # block by block on the oracle's inputs
    for i, p in enumerate(model.modules["blocks"]):
        xin = ref["trace"][p]
        want = TO.block(xin, p, cfg, W, ref["elen"], index=i)
        bar = 4 * _maxerr(TO.block(xin.float(), p, cfg, W, ref["elen"], torch.float32, index=i), want)
        figures[f"block_{i}_bar"] = bar
        for route in ("auto", "fused"):  # (auto: the unfused route for an f32 model unless the mask is causal)
            model.attention_route = route
            y = model.block_fwd(xin.float().to(dev).reshape(60, -1).contiguous(), p, 3, 20, lens_dev, i)
            model.attention_route = "auto"
            err = _maxerr(y.view(3, 20, -1).cpu(), want)
            figures[f"block_{i}_error_{route}"] = err
            assert err <= bar, (p, route, err, bar)
    # whole depth
    enc = _encode(model, ref, dev)
    err, bar = _maxerr(enc.cpu(), ref["enc"]), 4 * _maxerr(ref["enc32"], ref["enc"])
    figures.update(whole_depth_error=err, whole_depth_bar=bar)
    logits = K.matmul(enc.reshape(60, -1), model.ps.p2d("dec/logits/w"), bias=model.ps.p("dec/logits/b")).view(3, 20, 29)
    lerr, lbar = _maxerr(logits.cpu(), ref["logits"]), 4 * _maxerr(ref["logits32"], ref["logits"])
    figures.update(logits_error=lerr, logits_bar=lbar)
    print(variant, figures)
    _record(f"f32_{variant}", **figures)
    assert err <= bar and lerr <= lbar
    # the default route ("auto") of an f32 model is the unfused one unless the mask is causal; both routes meet the same bar
    assert model.attention_route == "auto"
    for route in ("fused",) + (() if cfg.use_attention_causal_mask else ("unfused",)):
        model.attention_route = route
        e2 = _encode(model, ref, dev)
        model.attention_route = "auto"
        err2 = _maxerr(e2.cpu(), ref["enc"])
        _record(f"f32_{variant}", **{f"whole_depth_error_{route}": err2})
        assert err2 <= bar, (route, err2, bar)


@pytest.mark.parametrize("variant", ["full", "chunked", "dh128"])
def test_bf16_whole_depth(dev, variant):
    ref = reference(variant)
    m16 = build(dev, variant, torch.bfloat16)
    enc = _encode(m16, ref, dev)
    assert enc.dtype == torch.bfloat16
    err, floor = _rel(enc.float().cpu(), ref["enc"]), _rel(ref["floor"], ref["enc"])
    print(f"{variant}: whole-depth bf16 relative error {err:.3e}, rounding floor {floor:.3e}")
    _record(f"bf16_{variant}", config=f"tiny {variant} (tests/test_transformer_gpu.py)", bf16_whole_depth_rel_error=err,
            bf16_rounding_floor=floor, allowed=2 * floor)
    assert floor > 0 and err <= 2 * floor


@pytest.mark.parametrize("setting", ["full", "chunked"])
def test_greedy_tokens_equal_the_oracles(models, audio, setting):
    """from the audio, no frame and no utterance excluded; tests/test_transformer_oracle.py asserts the margin on this fixture"""
    model, ref = models[setting], reference(setting)
    assert ref["margin"] >= 100 * ref["logit_err32"] and all(len(w) > 3 for w in ref["tokens"])
    x = _inputs(audio)
    logits, elen = model._infer_logits(x)
    assert list(elen) == C.ELEN and logits.shape == (3, 20, 29)
    greedy = model.recognize(x).tokens.cpu().numpy()
    for b in range(3):
        assert [int(v) for v in greedy[b] if v != 0] == ref["tokens"][b], b
    out = model(TrainInput(x.inputs, x.inputs_length, None, None))
    assert out.logits.shape == (3, 20, 29) and out.logits_length.tolist() == C.ELEN
    # a bf16 model decodes on its f32 twin by default: the same tokens
    m16 = build(model.device, setting, torch.bfloat16)
    assert torch.equal(m16.recognize(x).tokens.cpu(), torch.from_numpy(greedy))
    assert m16.encode(x.inputs, x.inputs_length)[0].dtype == torch.float32
    assert m16.encode(x.inputs, x.inputs_length, precision="bf16")[0].dtype == torch.bfloat16


def test_transducer_greedy_search_runs_on_the_transformer_frames(dev, audio):
    model = build(dev, "full", cls=TransformerTransducer, head="rnnt")
    cfg = model.cfg
    x = _inputs(audio)
    x = PredictInput(x.inputs, x.inputs_length, model.get_initial_tokens(3), None, model.get_initial_decoder_states(3))
    got = model.recognize(x)
    # the existing search on the ORACLE's encoder frames (computed from the oracle's features with this model's weights)
    ref = C.reference("full", cfg=cfg, W=C.make_weights(cfg))
    want = model.recognize_encoded(ref["enc"].float().to(dev).contiguous(), ref["elen"], x.previous_tokens, x.previous_decoder_states)
    assert torch.equal(got.tokens.cpu(), want.tokens.cpu()) and bool((got.tokens != 0).any())
    beam = model.recognize_beam(x, beam_width=4, device_search=True)
    toks, n, score, _, _ = model.recognize_beam_encoded(ref["enc"].float().to(dev).contiguous(), ref["elen"], 4, 1, x.previous_tokens,
                                                        x.previous_decoder_states)
    assert torch.equal(beam.tokens.cpu(), toks[:, 0].cpu()) and bool(torch.isfinite(score).all())
    with pytest.raises(ValueError):
        TransformerTransducer(C.tiny_config("full"), dev)
    with pytest.raises(ValueError):
        TransformerCTC(cfg, dev)


def test_beam_search_align_and_evaluate_agree_with_the_same_calls_on_the_logits(models, audio, tmp_path):
    model = models["full"]
    dev = model.device
    x = _inputs(audio)
    logits, elen = model._infer_logits(x)
    elen_dev = torch.tensor(elen, dtype=torch.int32, device=dev)
    bd = model.recognize_beam(x, beam_width=4, device_search=True).tokens.cpu()
    toks, n, _ = K.ctc_beam_search_device(logits, elen_dev, beam_width=4, top_paths=1, blank_index=None)
    assert torch.equal(bd, toks[:, 0, :max(int(n.max()), 1)].cpu())
    bh = model.recognize_beam(x, beam_width=4).tokens.cpu()
    assert torch.equal(bh[:, :bd.shape[1]], bd[:, :bh.shape[1]])
    nb, nlen, _ = model.recognize_nbest(x, beam_width=4, top_paths=2)
    assert torch.equal(nb[:, 0, :bd.shape[1]].cpu(), bd) and bool((nlen[:, 1] > 0).all())
    greedy = model.recognize(x).tokens.cpu()
    llen = (greedy != 0).sum(1).to(torch.int32)
    labels = torch.zeros_like(greedy)
    for b in range(3):
        labels[b, :llen[b]] = greedy[b][greedy[b] != 0]
    out = model.align(TrainData(TrainInput(x.inputs, x.inputs_length, None, None), TrainLabel(labels, llen)))
    start, end, label_lp, score = K.ctc_align(logits, labels.to(dev).to(torch.int32).contiguous(), llen.to(dev), elen_dev, blank=0)
    assert torch.equal(out.frames, start) and torch.equal(out.ends, end) and torch.equal(out.scores, score) and bool(torch.isfinite(score).all())
    for b in range(3):
        k = int(llen[b])
        assert bool((start[b, :k] >= 0).all()) and bool((end[b, :k] <= elen[b]).all()) and bool((start[b, :k] < end[b, :k]).all())
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
    rows = model.evaluate(ds, output_file_path=os.path.join(tmp_path, "result.tsv"), batch_size=2)
    g = rows["greedy"]
    assert g["utterances"] == 2 and g["wer"] == 0 and g["cer"] == 0 and g["ter"] == 0 and g["tokens"]["distance"] == 0


def test_npz_round_trip_under_the_references_names(dev, models, audio, tmp_path):
    model = models["chunked"]
    path = os.path.join(tmp_path, "transformer.npz")
    names = model.save_weights(path)
    for must in ("encoder/block_1/mhsa/attention_output/kernel", "encoder/block_0/mhsa/query/bias", "encoder/subsampling/block_1/bn_1/moving_mean",
                 "encoder/linear/kernel", "encoder/block_0/ln_2/gamma", "encoder/block_1/pwffn/ffn_1/kernel", "decoder/logits/kernel"):
        assert must in names, must
    with np.load(path) as z:
        assert z["encoder|block_0|mhsa|query|kernel"].shape == (64, 2, 64) and z["encoder|block_0|mhsa|attention_output|kernel"].shape == (2, 64, 64)
        assert z["encoder|block_0|mhsa|value|bias"].shape == (2, 64) and z["encoder|subsampling|block_0|conv_0|kernel"].shape == (3, 3, 1, 16)
    other = TransformerCTC(C.tiny_config("chunked"), dev, dtype=torch.float32, seed=11)
    x = _inputs(audio)
    before, _ = other._infer_logits(x)
    want, _ = model._infer_logits(x)
    assert not torch.equal(before, want)
    other.load_weights(path)  # (the folded BatchNorm pairs and packed kernels made for `before` must not survive the load)
    got, _ = other._infer_logits(x)
    assert torch.equal(got, want)
    with pytest.raises(NotImplementedError):
        model.save_weights(os.path.join(tmp_path, "transformer.weights.h5"))


def test_model_from_config_builds_both_classes_from_the_fixture(dev, audio):
    with open(C.CONFIG_FIXTURE) as f:
        fx = json.load(f)
    conf = dict(fx["base-streaming"]["config"], encoder_num_blocks=1, vocab_size=29)  # (one block of the shipped width keeps the test quick)
    m = base_model.model_from_config({"class_name": fx["base-streaming"]["class_name"], "config": conf}, device=dev)
    assert type(m) is TransformerCTC and m.dtype == torch.bfloat16 and (m.cfg.chunk_size, m.cfg.history_size, m.cfg.head_size) == (16, 64, 128)
    x = _inputs(audio)
    assert m.recognize(x).tokens.shape[0] == 3
    enc, elen = m.encode(x.inputs, x.inputs_length, precision="bf16")
    assert enc.shape == (3, 20, 512) and list(elen) == C.ELEN and bool(torch.isfinite(enc.float()).all())
    t = base_model.model_from_config({"class_name": "tensorflow_asr.models.transducer.transformer>Transformer",
                                      "config": dict(conf, prediction_rnn_units=64, prediction_embed_dim=32, joint_dim=48)}, device=dev)
    assert type(t) is TransformerTransducer and t.cfg.head == "transducer" and t.cfg.rnn_units == 64
    assert type(base_model.model_from_config(fx["base"], device=dev, dtype=torch.float32)) is TransformerCTC


def test_training_and_streaming_are_refused(models, audio):
    model = models["full"]
    x = _inputs(audio)
    data = TrainData(TrainInput(x.inputs, x.inputs_length, None, None), TrainLabel(torch.ones(3, 2, dtype=torch.int32), torch.tensor([2, 2, 2])))
    for call in (lambda: model.train_step(data), lambda: model.loss_and_backward(data), lambda: model.compile(), lambda: model.stream(),
                 lambda: model.stream_state(), lambda: model.encode_chunk(None, None, None)):
        with pytest.raises(NotImplementedError, match="inference only"):
            call()
    with pytest.raises(ValueError):
        TransformerCTC(configs.conformer_tiny(head="ctc"), model.device)
