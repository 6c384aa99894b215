"""The float64 DeepSpeech2 oracle (tests/ds2_oracle.py) pinned on the CPU: each layer against a direct restatement, and the whole encoder
against the reference's OWN DeepSpeech2Encoder class constructed and run over oracle/keras_shim.reference_runtime() (Conv2D "same" and
"causal", BatchNormalization, DepthwiseConv1D, the masked LSTM and the Keras mask plumbing are the shim's).  The shim's Bidirectional is
a stub: this module installs its own wrapper on the runtime's keras.layers namespace, as Keras documents the layer - a forward layer plus
a backward layer that sees the time-flipped sequence with the time-flipped mask, its output flipped back, the two concatenated.  The
reference runs are skipped where the reference tree is absent; the restatement tests always run."""
import importlib
import os

import numpy as np
import pytest
import torch

from oracle import keras_shim as KS
from tensorflowasr_amd import checkpoint

import ds2_cases as C
import ds2_oracle as DO

HAVE_REFERENCE = os.path.isdir(os.path.join(KS.REFERENCE_ROOT, "tensorflow_asr", "models", "encoders"))


# ------------------------------------------------------------------------------------------------------------ layer restatements
@pytest.mark.parametrize("padding", ["same", "causal"])
@pytest.mark.parametrize("kh,kw,st,sf,T,F", [(5, 7, 3, 2, 7, 16), (3, 5, 1, 2, 4, 9), (4, 6, 2, 1, 5, 8), (1, 1, 1, 2, 3, 7), (11, 3, 2, 2, 1, 2)])
def test_conv2d_against_the_definition(padding, kh, kw, st, sf, T, F):
    g = torch.Generator().manual_seed(kh * 100 + kw)
    x, w = torch.randn(2, T, F, 3, generator=g).double(), torch.randn(kh, kw, 3, 4, generator=g).double()
    y = DO.conv2d(x, w, (st, sf), padding)
    To, Fo = -(-T // st), -(-F // sf)
    assert y.shape == (2, To, Fo, 4)
    pt = kh - 1 if padding == "causal" else max((To - 1) * st + kh - T, 0) // 2
    pf = kw - 1 if padding == "causal" else max((Fo - 1) * sf + kw - F, 0) // 2
    want = torch.zeros(2, To, Fo, 4, dtype=torch.float64)
    for t in range(To):
        for f in range(Fo):
            for i in range(kh):
                for j in range(kw):
                    r, p = t * st + i - pt, f * sf + j - pf
                    if 0 <= r < T and 0 <= p < F:
                        want[:, t, f] += x[:, r, p] @ w[i, j]
    np.testing.assert_allclose(y.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)


def test_same_padding_is_what_the_shim_restates():
    """keras "same": the shim's _conv_nd (oracle/keras_shim.py) on the same operands"""
    g = torch.Generator().manual_seed(1)
    x, w = torch.randn(2, 9, 16, 2, generator=g), torch.randn(5, 7, 2, 3, generator=g)
    for strides in ((2, 2), (1, 2), (3, 1)):
        got = DO.conv2d(x, w, strides, "same").numpy()
        want = np.asarray(KS._conv_nd(x.numpy().astype(np.float64), w.numpy().astype(np.float64), strides, "same"), np.float64)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)


def test_masked_lstm_and_its_reverse():
    g = torch.Generator().manual_seed(2)
    B, T, P = 4, 6, 5
    xg, rk = torch.randn(B, T, 4 * P, generator=g).double(), torch.randn(P, 4 * P, generator=g).double() * 0.4
    lens = [6, 1, 0, 3]
    y, h, c = DO.lstm(xg, rk, lens)
    for b, n in enumerate(lens):
        assert not y[b, n:].any()
        y1, h1, c1 = DO.lstm(xg[b:b + 1, :max(n, 1)], rk, [n])  # the row alone, cut at its length: the same chain
        np.testing.assert_allclose(y[b, :n].numpy(), y1[0, :n].numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(h[b].numpy(), h1[0].numpy(), rtol=1e-12, atol=1e-14)
        if n:
            np.testing.assert_allclose(h[b].numpy(), y[b, n - 1].numpy(), rtol=1e-12, atol=1e-14)  # the state at the last valid step
        else:
            assert not h[b].any() and not c[b].any()
    # reverse = flip sequence AND mask, run forward, flip back (keras Bidirectional's backward layer)
    yr, hr, cr = DO.lstm(xg, rk, lens, reverse=True)
    for b, n in enumerate(lens):
        xf = xg[b:b + 1, :max(n, 1)].flip(1)
        y1, h1, c1 = DO.lstm(xf, rk, [n])
        np.testing.assert_allclose(yr[b, :n].numpy(), y1[0, :n].flip(0).numpy(), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(cr[b].numpy(), c1[0].numpy(), rtol=1e-12, atol=1e-14)
        assert not yr[b, n:].any()
    y2, h2, c2 = DO.lstm_infer(torch.cat([xg, xg], -1), torch.stack([rk, rk]), lens, 2)
    assert torch.equal(y2[:, :, :P], y) and torch.equal(y2[:, :, P:], yr) and torch.equal(h2[1], hr) and torch.equal(c2[0], c)


def test_rowconv_is_causal():
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(2, 7, 3, generator=g).double(), torch.randn(5, 3, generator=g).double()
    y = DO.rowconv(x, w)
    want = torch.zeros_like(x)
    for t in range(7):
        for k in range(5):
            if t - 4 + k >= 0:
                want[:, t] += w[k] * x[:, t - 4 + k]
    np.testing.assert_allclose(y.numpy(), want.numpy(), rtol=1e-12, atol=1e-12)


def test_spectrogram_against_a_direct_dft():
    cfg = C.tiny_config("bi", num_feature_bins=160)
    sig = C.audio()[:1, :1000]
    feat = DO.spectrogram(sig, cfg)
    assert feat.shape == (1, 7, 160)
    x = np.concatenate([sig[0, :1], sig[0, 1:] - np.float32(0.97) * sig[0, :-1]]).astype(np.float64)
    x = np.pad(x, (0, 6 * 160 + 400 - 1000))
    n = np.arange(400)
    window = 0.5 - 0.5 * np.cos(2 * np.pi * n / 400)
    for t in (0, 6):
        fr = x[t * 160:t * 160 + 400] * window
        dft = np.array([np.sum(fr * np.exp(-2j * np.pi * k * n / 512)) for k in range(160)])
        np.testing.assert_allclose(feat[0, t].numpy(), np.log(np.abs(dft) ** 2 + 1e-6), atol=2e-5, rtol=0)


@pytest.mark.parametrize("variant", ["bi", "uni"])
def test_the_chosen_seeds_meet_the_conditions_on_the_input(variant):
    """tests/test_ds2_gpu.py compares greedy tokens: the oracle's top-two logit margin exceeds 1e-3 on every valid frame, and every
    utterance says more than three tokens"""
    ref = C.reference(variant, C.audio())
    assert ref["elen"] == [16, 25, 40] and ref["margin"] > 1e-3 and all(len(t) > 3 for t in ref["tokens"])
    assert all(m.shape == (3, 40) and m.sum(1).tolist() == [16, 25, 40] for m in ref["trace"]["masks"])
    assert len(ref["trace"]["masks"]) == (4 if variant == "bi" else 2)


# ------------------------------------------------------------------------------------------------------------ the reference's classes
def _bidirectional(tf):
    class Bidirectional(KS.Layer):
        """keras.layers.Bidirectional(merge_mode="concat") over the shim's LSTM: `layer` becomes forward_<name>, a second layer of the
        same configuration backward_<name>; the backward layer walks the time-reversed sequence with the time-reversed mask and its
        output is reversed back (keras: go_backwards=True, then reverse on the time axis)."""

        def __init__(self, layer, merge_mode="concat", name=None, dtype=None, **kwargs):
            super().__init__(name=name)
            assert merge_mode == "concat" and isinstance(layer, KS.LSTM)
            base = layer.name
            self.forward_layer = layer
            self.backward_layer = KS.LSTM(layer.units, return_sequences=layer.return_sequences, return_state=layer.return_state,
                                          zero_output_for_mask=layer.zero_output_for_mask, kernel_regularizer=layer.kernel_regularizer,
                                          bias_regularizer=layer.bias_regularizer, name="backward_" + base)
            layer.name = "forward_" + base
            self.supports_masking = True

        def call(self, sequences, mask=None, training=False):
            yf, *sf = self.forward_layer(sequences, mask=mask)
            xr = tf.convert_to_tensor(np.asarray(sequences)[:, ::-1].copy())
            mr = None if mask is None else np.asarray(mask)[:, ::-1].copy()
            yb, *sb = self.backward_layer(xr, mask=mr)
            y = tf.convert_to_tensor(np.concatenate([np.asarray(yf), np.asarray(yb)[:, ::-1]], -1))
            return (y, *sf, *sb)

        def compute_mask(self, _, mask):
            return [mask, None, None, None, None]

    return Bidirectional


@pytest.mark.skipif(not HAVE_REFERENCE, reason="the reference tree is not on this machine")
@pytest.mark.parametrize("variant", ["uni", "bi"])
def test_encoder_against_the_references_own_class(variant):
    cfg = C.tiny_config(variant)
    W = C.make_weights(cfg)
    sig = C.audio()
    feats = DO.spectrogram(sig, cfg).float()
    flen = [-(-n // cfg.frame_step) for n in C.SAMPLES]
    arrays = checkpoint.to_keras({k: v for k, v in W.items() if k.startswith("enc/")}, path_fn=checkpoint.deepspeech2_keras_path)
    with KS.reference_runtime() as (tf, keras):
        keras.layers.Bidirectional = _bidirectional(tf)
        mod = importlib.import_module("tensorflow_asr.models.encoders.deepspeech2")
        enc = mod.DeepSpeech2Encoder(conv_type=cfg.conv_type, conv_kernels=cfg.conv_kernels, conv_strides=cfg.conv_strides,
                                     conv_filters=cfg.conv_filters, conv_padding=cfg.conv_padding, conv_activation=cfg.conv_activation,
                                     rnn_nlayers=cfg.rnn_nlayers, rnn_type=cfg.rnn_type, rnn_units=cfg.rnn_units,
                                     rnn_bidirectional=cfg.rnn_bidirectional, rnn_rowconv=cfg.rnn_rowconv,
                                     rnn_rowconv_activation=cfg.rnn_rowconv_activation, fc_nlayers=cfg.fc_nlayers, fc_units=cfg.fc_units,
                                     fc_activation=cfg.fc_activation, name="encoder")
        inputs = (tf.convert_to_tensor(feats.numpy()[..., None]), tf.convert_to_tensor(np.asarray(flen, np.int32)))
        enc(inputs, training=False)  # builds every variable
        named = enc.named_weights()
        assert sorted(named) == sorted(arrays)  # the parameter set under the reference's own layer names
        for path, var in named.items():
            assert tuple(var.shape) == arrays[path].shape, path
            var.assign(arrays[path])
        for blk in enc.rnn_module.blocks:
            for lyr in ([blk.rnn.forward_layer, blk.rnn.backward_layer] if cfg.rnn_bidirectional else [blk.rnn]):
                del lyr.masks_seen[:]
        out, out_len = enc(inputs, training=False)
        out, out_len = np.asarray(out, np.float64), np.asarray(out_len).tolist()
        seen = []
        for blk in enc.rnn_module.blocks:
            for lyr in ([blk.rnn.forward_layer, blk.rnn.backward_layer] if cfg.rnn_bidirectional else [blk.rnn]):
                assert len(lyr.masks_seen) == 1
                seen.append(lyr.masks_seen[0])
        assert enc.time_reduction_factor == cfg.time_reduction_factor
    trace = {}
    want, elen = DO.encoder(feats, flen, cfg, W, trace=trace)
    assert out_len == elen == [16, 25, 40]
    # the shim computes in float64 and stores float32 between layers
    np.testing.assert_allclose(out, want.numpy(), rtol=1e-5, atol=1e-6)
    # the masks the LSTMs saw: sequence_mask(conv-reduced length) - flipped for a backward layer, which sees the flipped sequence
    assert len(seen) == len(trace["masks"])
    for k, (got, m) in enumerate(zip(seen, trace["masks"])):
        m = m.numpy()
        backward = cfg.rnn_bidirectional and k % 2 == 1
        assert got is not None and np.array_equal(np.asarray(got, bool), m[:, ::-1] if backward else m), k
    # padded frames of a short row are NOT what the utterance alone gives under "same" + bidirectional, and are under causal + forward
    one, _ = DO.encoder(feats[:1, :flen[0]], flen[:1], cfg, W)
    same = np.allclose(one[0, :elen[0]].numpy(), want[0, :elen[0]].numpy(), rtol=1e-9, atol=1e-12)
    assert same == (variant == "uni")
