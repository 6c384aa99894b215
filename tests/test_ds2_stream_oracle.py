"""What a DeepSpeech2 stream carries, pinned on the CPU in float64 (tests/ds2_stream_oracle.py), and where that departs from the
reference's own call_next.

1. The unidirectional encoder fed in pieces, with the conv blocks' input tails, the LSTM states and the RowConv1D tails carried, gives
   ds2_oracle.encoder of the whole utterance to 1e-12 for every chunking: that is the state a session needs, no more.
2. The reference's DeepSpeech2Encoder.call_next (run over oracle/keras_shim, skipped where the reference tree is absent) carries the LSTM
   states ONLY and pads every chunk's convolutions and RowConv1Ds afresh.  Its states are the ones the restatement carries, in the
   [B, nlayers, 2, P] (h, c) layout; its first chunk is the offline output; its second chunk is NOT the offline output - it is the
   restatement with the tails dropped - which is the departure the session documents."""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import keras_shim as KS
from tensorflowasr_amd import checkpoint

import ds2_cases as C
import ds2_oracle as DO
import ds2_stream_oracle as SO

HAVE_REFERENCE = os.path.isdir(os.path.join(KS.REFERENCE_ROOT, "tensorflow_asr", "models", "encoders"))


@pytest.fixture(scope="module")
def case():
    cfg = C.tiny_config("uni")
    W = C.make_weights(cfg)
    feats = DO.spectrogram(C.audio(), cfg)
    flen = [-(-n // cfg.frame_step) for n in C.SAMPLES]
    enc, elen = DO.encoder(feats, flen, cfg, W)
    return cfg, W, feats, flen, enc, elen


def _pieces(n, how):
    if how == "ragged":  # multiples of the time reduction factor 2 of every size, then whatever is left
        sizes, k = [], 0
        while sum(sizes) < n:
            sizes.append(min([2, 10, 4, 2, 16, 6][k % 6], n - sum(sizes)))
            k += 1
        return sizes
    return [min(how, n - t) for t in range(0, n, how)]


@pytest.mark.parametrize("how", [8, 2, "ragged"])
def test_chunked_restatement_is_the_offline_encoder(case, how):
    cfg, W, feats, flen, enc, elen = case
    for b, n in enumerate(flen):  # 31 (odd), 50 and 80 feature frames
        ce = SO.ChunkedEncoder(cfg, W)
        out, t = [], 0
        for size in _pieces(n, how):
            out.append(ce.step(feats[b, t:t + size]))
            t += size
        got = torch.cat(out)
        assert got.shape == (elen[b], cfg.dmodel)
        np.testing.assert_allclose(got.numpy(), enc[b, :elen[b]].numpy(), rtol=0, atol=1e-12)
        assert tuple(ce.states().shape) == (1, cfg.rnn_nlayers, 2, cfg.rnn_units)


def test_dropping_a_tail_changes_the_frames_behind_the_cut(case):
    """the carried tails are needed: without the conv tails or without the RowConv1D tails the second piece is not the offline output"""
    cfg, W, feats, flen, enc, elen = case
    for drop in ("conv_tails", "row_tails"):
        ce = SO.ChunkedEncoder(cfg, W)
        first = ce.step(feats[2, :40])
        setattr(ce, drop, [None] * len(getattr(ce, drop)))
        second = ce.step(feats[2, 40:80])
        np.testing.assert_allclose(first.numpy(), enc[2, :20].numpy(), rtol=0, atol=1e-12)
        assert float((second - enc[2, 20:40]).abs().max()) > 1e-3, drop


@pytest.mark.skipif(not HAVE_REFERENCE, reason="the reference tree is not on this machine")
def test_the_references_call_next_carries_the_lstm_states_only(case):
    cfg, W, feats, flen, enc, elen = case
    arrays = checkpoint.to_keras({k: v for k, v in W.items() if k.startswith("enc/")}, path_fn=checkpoint.deepspeech2_keras_path)
    x = feats[2:3, :80].float().numpy()[..., None]  # the 0.8 s utterance alone, in two chunks of 40 feature frames
    with KS.reference_runtime() as (tf, keras):
        mod = importlib.import_module("tensorflow_asr.models.encoders.deepspeech2")
        ref = mod.DeepSpeech2Encoder(conv_type=cfg.conv_type, conv_kernels=cfg.conv_kernels, conv_strides=cfg.conv_strides,
                                     conv_filters=cfg.conv_filters, conv_padding=cfg.conv_padding, conv_activation=cfg.conv_activation,
                                     rnn_nlayers=cfg.rnn_nlayers, rnn_type=cfg.rnn_type, rnn_units=cfg.rnn_units,
                                     rnn_bidirectional=cfg.rnn_bidirectional, rnn_rowconv=cfg.rnn_rowconv,
                                     rnn_rowconv_activation=cfg.rnn_rowconv_activation, fc_nlayers=cfg.fc_nlayers, fc_units=cfg.fc_units,
                                     fc_activation=cfg.fc_activation, name="encoder")
        ref((tf.convert_to_tensor(x), tf.convert_to_tensor(np.asarray([80], np.int32))), training=False)  # builds every variable
        for path, var in ref.named_weights().items():
            var.assign(arrays[path])
        s0 = ref.get_initial_state(batch_size=1)
        assert tuple(np.asarray(s0).shape) == (1, cfg.rnn_nlayers, 2, cfg.rnn_units) and not np.asarray(s0).any()
        y1, n1, s1 = ref.call_next(tf.convert_to_tensor(x[:, :40]), tf.convert_to_tensor(np.asarray([40], np.int32)), s0)
        y2, n2, s2 = ref.call_next(tf.convert_to_tensor(x[:, 40:]), tf.convert_to_tensor(np.asarray([40], np.int32)), s1)
        y1, y2, s1, s2 = (np.asarray(v, np.float64) for v in (y1, y2, s1, s2))
        assert np.asarray(n1).tolist() == np.asarray(n2).tolist() == [20]
    bar = dict(rtol=1e-5, atol=1e-6)  # the shim computes in float64 and stores float32 between layers (tests/test_ds2_oracle.py)
    carried = SO.ChunkedEncoder(cfg, W)   # what the session carries: tails and states
    states_only = SO.ChunkedEncoder(cfg, W)  # what call_next carries
    c1, r1 = carried.step(feats[2, :40]), states_only.step(feats[2, :40])
    # the first chunk: zeros in front of it ARE the causal padding, so call_next, both restatements and the offline run agree ...
    np.testing.assert_allclose(y1[0], enc[2, :20].numpy(), **bar)
    np.testing.assert_allclose(c1.numpy(), r1.numpy(), rtol=0, atol=0)
    # ... and its states are the ones the restatement carries, in the reference's layout
    assert s1.shape == s2.shape == (1, cfg.rnn_nlayers, 2, cfg.rnn_units)
    np.testing.assert_allclose(s1, carried.states().numpy(), **bar)
    states_only.conv_tails, states_only.row_tails = [None] * len(states_only.conv_tails), [None] * len(states_only.row_tails)
    c2, r2 = carried.step(feats[2, 40:80]), states_only.step(feats[2, 40:80])
    # the second chunk: call_next is the restatement WITHOUT the tails, and that is not the offline output; with the tails it is
    np.testing.assert_allclose(y2[0], r2.numpy(), **bar)
    np.testing.assert_allclose(s2, states_only.states().numpy(), **bar)
    np.testing.assert_allclose(c2.numpy(), enc[2, 20:40].numpy(), rtol=0, atol=1e-12)
    gap = np.abs(y2[0] - enc[2, 20:40].numpy()).max(-1)  # per encoder frame
    # the fresh padding reaches the chunk's first frames directly: 2 frames of conv block 0 (kh 5, stride 2), 2 more through block 1 (kh 3)
    # and the 2w = 4 behind them in every RowConv1D; the recurrence hands what it saw there on to the frames behind, fading
    assert gap[:4].max() > 1e-2 and gap[:4].max() > 10 * bar["atol"]
    assert gap[:8].max() >= gap[12:].max()
    np.testing.assert_allclose(carried.states().numpy()[0, :, 0], np.stack([h[0].numpy() for h, _ in carried.hc]), rtol=0, atol=0)
