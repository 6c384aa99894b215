"""RnnTransducer (tensorflowasr_amd/rnnt.py) on the GPU against the recorded run of the reference's own classes
(tests/golden/rnnt_wiring.npz) and the float64 oracle of tests/rnnt_oracle.py, and the wiring of the inherited decoders, alignment,
evaluation and checkpoints.

Tiny model (tests/rnnt_cases.py): F = 16 mel bins, rnn_units 32, dmodel 16, V = 29; "ln" = three blocks, reductions [post, post, pre] by
[3, 0, 2] with LayerNorm, "noln" = two blocks, [pre, pre] by [2, 0] without; one batch of 31 / 50 / 80 feature frames.

Bars, as tests/test_ds2_gpu.py sets them.  f32: the project's single-layer bar (rtol 1e-4 / atol 1e-5) times the number of layers in the
chain - every block is a recurrence and a tail - plus, against the recorded run, that run's own distance from the f64 oracle (it stores
float32 between layers).  bf16: the relative error against the f64 oracle may be twice the rounding floor, a float64 CPU run that rounds
the features, the kernels and every stored activation to bf16.  Every row is compared, padded ones included: behind a `post` reduction
they are live."""
import json
import os

import numpy as np
import pytest
import torch

from tensorflowasr_amd import base_model, configs
from tensorflowasr_amd import tokenizers as tk
from tensorflowasr_amd.datasets import ASRSliceDataset
from tensorflowasr_amd.rnnt import RnnTransducer
from tensorflowasr_amd.schemas import PredictInput, TrainData, TrainInput, TrainLabel

import rnnt_cases as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "librispeech", "characters", "english.vocab")
F32_BAR = dict(rtol=1e-4, atol=1e-5)  # the project's single-layer bar (tests/test_ds2_gpu.py)
SAMPLES = C.SAMPLES


def build(dev, setting="ln", dtype=torch.float32, **over):
    cfg = C.tiny_config(setting, **over)
    model = RnnTransducer(cfg, dev, dtype=dtype, seed=3)
    model.ps.import_keras(C.make_weights(cfg))
    model.tokenizer = tk.get({"type": "characters", "blank_index": 0, "vocabulary": VOCAB})
    return model


@pytest.fixture(scope="module")
def audio():
    return C.audio()


@pytest.fixture(scope="module")
def models(dev):
    return {s: build(dev, s) for s in C.SETTINGS}


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
    """the encoder on the fixture's features (the same operands), every row"""
    feats = torch.from_numpy(ref["feats"]).to(model.dtype).to(dev).contiguous()
    x, T, lens, lens_dev = model.encoder_fwd(feats, ref["flen"], False, None)
    torch.cuda.synchronize()
    assert lens == ref["elen"] == lens_dev.cpu().tolist() and T == max(ref["elen"])
    return x.view(3, T, -1)


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_load_weights_of_the_wiring_fixture_reproduces_the_recorded_run(dev, setting, tmp_path):
    with np.load(C.WIRING) as z:
        wiring = {k: z[k] for k in z.files}
    ref = C.reference(setting)
    cfg = ref["cfg"]
    model = RnnTransducer(cfg, dev, dtype=torch.float32, seed=99)
    path = os.path.join(tmp_path, "wiring.npz")
    pre = f"{setting}|w|"
    with open(path, "wb") as f:  # the fixture's encoder weights as a checkpoint file under the reference's names
        np.savez(f, **{k[len(pre):]: v for k, v in wiring.items() if k.startswith(pre)})
    names = model.load_weights(path, skip_mismatch=True)  # (the fixture holds the encoder only: the head keeps its initial values)
    assert "enc/block_1/lstm/rk" in names and len(names) == (7 if cfg.layer_norm else 5) * cfg.nlayers
    assert np.array_equal(wiring["feats"], ref["feats"])
    enc = _encode(model, ref, dev)
    want = wiring[f"{setting}|encoder"]
    n = 2 * cfg.nlayers
    err = np.abs(enc.cpu().numpy().astype(np.float64) - want)
    bar = n * (F32_BAR["atol"] + F32_BAR["rtol"] * np.abs(want)) + _maxerr(want, ref["enc"])
    print(f"{setting}: against the recorded reference run: {err.max():.3e} (bar {bar.min():.3e} .. {bar.max():.3e})")
    assert (err <= bar).all()


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_blocks_and_whole_depth_against_the_oracle_f32(dev, models, setting):
    import rnnt_oracle as RO

    model, ref = models[setting], C.reference(setting)
    cfg = ref["cfg"]
    # block by block on the oracle's inputs: recurrence + tail = two layers
    for i, m in enumerate(model.modules):
        xin, lens = ref["trace"][m["name"]]
        want, _, _ = RO.block(xin, lens, m, ref["Wn"])
        sub = RnnTransducer.__new__(RnnTransducer)
        sub.__dict__.update(model.__dict__)
        sub.modules = [dict(m)]
        x, T, out_lens, _ = _run_block(sub, xin, lens, dev)
        assert out_lens == RO.block(xin, lens, m, ref["Wn"])[1]
        np.testing.assert_allclose(x.cpu().numpy(), want, rtol=2 * F32_BAR["rtol"], atol=2 * F32_BAR["atol"], err_msg=m["name"])
    enc = _encode(model, ref, dev)
    n = 2 * cfg.nlayers
    np.testing.assert_allclose(enc.cpu().numpy(), ref["enc"], rtol=n * F32_BAR["rtol"], atol=n * F32_BAR["atol"])
    # "auto" is the two-launch tail (tfasr_layernorm_fwd + tfasr_gemm + zero fill), the faster route as measured
    # (profiles/rnnt_timing.json); each route, named, meets the same bar
    assert model.tail_route == "auto" and not any(model._fused_tail(m) for m in model.modules)
    for route in ("fused", "unfused"):
        model.tail_route = route
        try:
            assert all(model._fused_tail(m) == (route == "fused" and m["ln"]) for m in model.modules)
            enc2 = _encode(model, ref, dev)
        finally:
            model.tail_route = "auto"
        np.testing.assert_allclose(enc2.cpu().numpy(), ref["enc"], rtol=n * F32_BAR["rtol"], atol=n * F32_BAR["atol"], err_msg=route)


def _run_block(sub, xin, lens, dev):
    """one block as a one-block encoder: encoder_fwd on the block's input rows"""
    x = torch.from_numpy(np.asarray(xin, np.float32)).to(dev).contiguous()
    out, T, out_lens, lens_dev = sub.encoder_fwd(x, lens, False, None)
    return out.view(x.shape[0], T, -1), T, out_lens, lens_dev


@pytest.mark.parametrize("setting,route", [("ln", "fused"), ("ln", "unfused"), ("noln", "unfused")])
def test_bf16_whole_depth(dev, setting, route):
    """both tail routes store what the floor rounds: the LSTM's output, the normalised rows (in LDS / in HBM), the block's output"""
    ref = C.reference(setting)
    m16 = build(dev, setting, torch.bfloat16)
    m16.tail_route = route
    assert all(m16._fused_tail(m) == (route == "fused") for m in m16.modules)
    enc = _encode(m16, ref, dev)
    assert enc.dtype == torch.bfloat16
    err, floor = _rel(enc.float().cpu(), ref["enc"]), _rel(ref["floor"], ref["enc"])
    print(f"{setting} {route}: whole-depth bf16 relative error {err:.3e}, rounding floor {floor:.3e}")
    path = os.path.join(ROOT, "profiles", "rnnt_parity.json")
    rec = {}
    if os.path.exists(path):
        with open(path) as f:
            rec = json.load(f)
    rec[f"bf16_{setting}_{route}"] = dict(config=f"tiny {setting}, tail route {route} (tests/test_rnnt_model_gpu.py)", bf16_whole_depth_rel_error=err, bf16_rounding_floor=floor,
                                  allowed=2 * floor)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    assert floor > 0 and err <= 2 * floor


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_greedy_tokens_equal_the_oracles(models, audio, setting):
    """from the audio; the batch through recognize_batch, each utterance alone through recognize_single"""
    model, ref = models[setting], C.reference(setting)
    x = _inputs(audio)
    x = PredictInput(x.inputs, x.inputs_length, model.get_initial_tokens(3), None, model.get_initial_decoder_states(3))
    enc, elen = model.encode(x.inputs, x.inputs_length)
    assert list(elen) == ref["elen"] and enc.shape == (3, max(ref["elen"]), model.cfg.dmodel) and enc.dtype == torch.float32
    greedy = model.recognize(x).tokens.cpu().numpy()
    for b in range(3):
        assert [int(v) for v in greedy[b] if v != 0] == ref["tokens"][b], b
        one = _inputs(audio, [b])
        got = model.recognize(PredictInput(one.inputs, one.inputs_length, model.get_initial_tokens(1), None, model.get_initial_decoder_states(1)))
        assert [int(v) for v in got.tokens[0].cpu().numpy() if v != 0] == ref["tokens_alone"][b], b
    # a bf16 model decodes on its f32 twin by default: the same tokens
    m16 = build(model.device, setting, torch.bfloat16)
    assert torch.equal(m16.recognize(x).tokens.cpu(), torch.from_numpy(greedy))
    assert m16.encode(x.inputs, x.inputs_length)[0].dtype == torch.float32
    assert m16.encode(x.inputs, x.inputs_length, precision="bf16")[0].dtype == torch.bfloat16


def test_beam_search_align_and_evaluate_agree_with_their_host_counterparts(models, audio, tmp_path):
    model = models["ln"]
    dev, cfg = model.device, model.cfg
    assert model.time_reduction_factor == 6 and abs(model.seconds_per_frame - 0.06) < 1e-12
    x = _inputs(audio)
    x = PredictInput(x.inputs, x.inputs_length, model.get_initial_tokens(3), None, model.get_initial_decoder_states(3))
    enc, elen = model.encode(x.inputs, x.inputs_length)
    # the searches on the model's own frames
    got = model.recognize(x)
    want = model.recognize_encoded(enc, elen, x.previous_tokens, x.previous_decoder_states)
    assert torch.equal(got.tokens.cpu(), want.tokens.cpu()) and bool((got.tokens != 0).any())
    assert torch.equal(model.recognize_beam(x, beam_width=4).tokens.cpu(), got.tokens.cpu())  # the host route is the greedy search
    beam = model.recognize_beam(x, beam_width=4, device_search=True)
    toks, n, score, _, _ = model.recognize_beam_encoded(enc, elen, 4, 1, x.previous_tokens, x.previous_decoder_states)
    assert torch.equal(beam.tokens.cpu(), toks[:, 0].cpu()) and bool(torch.isfinite(score).all()) and bool((n[:, 0] > 0).all())
    nb, nlen, nscore = model.recognize_nbest(x, beam_width=4, top_paths=2)
    assert torch.equal(nb[:, 0].cpu(), toks[:, 0].cpu()) and bool((nlen[:, 1] > 0).all()) and bool((nscore[:, 0] >= nscore[:, 1]).all())
    # alignment of the beam's best path: align() = align_encoded() on the same frames
    L = int(n[:, 0].max())
    labels = toks[:, 0, :L].cpu().to(torch.int32)
    llen = n[:, 0].cpu().to(torch.int32)
    pred = torch.cat([torch.zeros(3, 1, dtype=torch.int32), labels], 1)
    data = TrainData(TrainInput(x.inputs, x.inputs_length, pred, llen + 1), TrainLabel(labels, llen))
    out = model.align(data)
    out2 = model.align_encoded(enc, elen, pred, labels, llen)
    assert torch.equal(out.frames, out2.frames) and torch.equal(out.scores, out2.scores) and bool(torch.isfinite(out.scores).all())
    for b in range(3):
        k = int(llen[b])
        fr = out.frames[b, :k].cpu()
        assert bool((fr >= 0).all()) and bool((fr < elen[b]).all()) and bool((fr[1:] >= fr[:-1]).all())
    # a two-utterance .tsv whose transcripts are the model's own greedy ones: zero errors, and the results file is written
    greedy = got.tokens.cpu()
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
    # (utterance 2 is the longest of both batches: rows 1 and 2 are padded alike in the batch of three and in evaluate's batch of two)
    g = rows["greedy"]
    assert g["utterances"] == 2 and g["wer"] == 0 and g["cer"] == 0 and g["ter"] == 0 and g["tokens"]["distance"] == 0
    assert os.path.exists(os.path.join(tmp_path, "result.tsv"))


def test_npz_round_trip_under_the_references_names(dev, models, audio, tmp_path):
    model = models["ln"]
    path = os.path.join(tmp_path, "rnnt.npz")
    names = model.save_weights(path)
    for must in ("encoder/block_0/lstm/kernel", "encoder/block_1/lstm/recurrent_kernel", "encoder/block_2/lstm/bias", "encoder/block_1/ln/gamma",
                 "encoder/block_1/ln/beta", "encoder/block_2/projection/kernel", "encoder/block_0/projection/bias", "joint/enc/kernel"):
        assert must in names, must
    with np.load(path) as z:
        assert z["encoder|block_1|lstm|kernel"].shape == (48, 128) and z["encoder|block_2|projection|kernel"].shape == (32, 16)
    other = RnnTransducer(C.tiny_config("ln"), dev, dtype=torch.bfloat16, seed=11)
    x = _inputs(audio)
    want, _ = model.encode(x.inputs, x.inputs_length)
    before, _ = other.encode(x.inputs, x.inputs_length)
    b16, _ = other.encode(x.inputs, x.inputs_length, precision="bf16")  # (packs the projection kernels of the initial weights)
    assert not torch.equal(before, want)
    other.load_weights(path)
    got, _ = other.encode(x.inputs, x.inputs_length)
    assert torch.equal(got, want)
    a16, _ = other.encode(x.inputs, x.inputs_length, precision="bf16")  # the packed kernels made for `b16` must not survive the load
    assert not torch.equal(a16, b16) and _rel(a16.float().cpu(), want.cpu()) < 0.1


def test_model_from_config_builds_the_class_from_the_fixture(dev, audio):
    with open(C.CONFIG_FIXTURE) as f:
        fx = json.load(f)
    conf = dict(fx["config"], encoder_nlayers=2, encoder_reduction_positions=["post", "post"], encoder_reduction_factors=[3, 2],
                prediction_rnn_units=64, prediction_embed_dim=32, vocab_size=29)  # (two blocks of the shipped width keep the test quick)
    m = base_model.model_from_config({"class_name": fx["class_name"], "config": conf}, device=dev)
    assert type(m) is RnnTransducer and m.dtype == torch.bfloat16 and m.cfg.encoder_rnn_units == 1024 and m.cfg.dmodel == 640
    x = _inputs(audio)
    enc, elen = m.encode(x.inputs, x.inputs_length, precision="bf16")
    assert enc.shape == (3, 14, 640) and list(elen) == [6, 9, 14] and bool(torch.isfinite(enc.float()).all())
    x = PredictInput(x.inputs, x.inputs_length, m.get_initial_tokens(3), None, m.get_initial_decoder_states(3))
    assert m.recognize(x).tokens.shape[0] == 3


def test_training_is_refused_and_wrong_configs_too(models, audio):
    model = models["ln"]
    x = _inputs(audio)
    data = TrainData(TrainInput(x.inputs, x.inputs_length, None, None), TrainLabel(torch.ones(3, 2, dtype=torch.int32), torch.tensor([2, 2, 2])))
    for call in (lambda: model.train_step(data), lambda: model.loss_and_backward(data), lambda: model.compile()):
        with pytest.raises(NotImplementedError, match="inference only"):
            call()
    with pytest.raises(ValueError):
        RnnTransducer(configs.conformer_tiny(), model.device)
