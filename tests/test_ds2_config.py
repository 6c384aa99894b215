"""DeepSpeech2 CTC without a device: the config surface against the rendered reference YAMLs (tests/golden/deepspeech2_config.json, made
by tools/render_deepspeech2_config.py), lengths, the parameter set under the reference's layer names, the spectrogram band table, the
model registry, and the host-side argument checks of the new entry points (csrc/conv2d_gen.hip, csrc/lstm_infer.hip)."""
import ctypes
import dataclasses
import json
import os
import re

import numpy as np
import pytest

from tensorflowasr_amd import _lib, checkpoint, configs, params

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID, UNSUPPORTED = 1, _lib.STATUS_UNSUPPORTED


def _fixture():
    with open(os.path.join(HERE, "golden", "deepspeech2_config.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("variant", ["base", "uni"])
def test_reference_yaml_equals_the_shipped_config_field_by_field(variant):
    fx = _fixture()[variant]
    assert fx["class_name"] == "tensorflow_asr.models.ctc.deepspeech2>DeepSpeech2"
    got, want = configs.deepspeech2_from_reference(fx["config"]), configs.deepspeech2(vocab_size=1000, variant=variant)
    for f in dataclasses.fields(configs.DeepSpeech2Config):
        assert getattr(got, f.name) == getattr(want, f.name), f.name
    assert got.feature_type == "spectrogram" and got.num_feature_bins == 160 and got.rnn_units == 512 and got.fc_units == 1024
    assert got.conv_kernels == [[11, 41], [11, 21]] and got.conv_strides == [[2, 2], [1, 2]] and got.conv_filters == [32, 32]
    assert got.time_reduction_factor == 2 and got.rnn_in == 40 * 32 and got.dmodel == 1024
    if variant == "base":
        assert got.conv_padding == "same" and got.rnn_bidirectional and not got.has_rowconv and got.ndir == 2 and got.rnn_out == 1024
    else:
        assert got.conv_padding == "causal" and not got.rnn_bidirectional and got.has_rowconv and got.rnn_rowconv == 3 and got.rnn_out == 512


def test_class_defaults_are_the_constructors():
    """models/ctc/deepspeech2.py:63-83: three conv blocks, time stride 3, 1024 units, no FC"""
    c = configs.DeepSpeech2Config()
    assert c.conv_strides == [[3, 2], [1, 2], [1, 2]] and c.conv_filters == [32, 32, 96] and c.rnn_units == 1024 and c.fc_nlayers == 0
    assert c.time_reduction_factor == 3 and c.dmodel == 2048 and c.rnn_in == 10 * 96


def test_spectrogram_is_deepspeech2s_alone():
    sc = _fixture()["base"]["config"]["speech_config"]
    with pytest.raises(NotImplementedError):
        configs.ConformerConfig.from_reference({"speech_config": sc})
    with pytest.raises(NotImplementedError):
        configs.speech_kwargs(sc)
    assert configs.speech_kwargs(sc, feature_types=("log_mel_spectrogram", "spectrogram"))["num_feature_bins"] == 160


@pytest.mark.parametrize("over", [dict(conv_type="conv1d"), dict(rnn_type="gru"), dict(rnn_type="rnn"), dict(conv_activation="silu"),
                                  dict(fc_activation="tanh"), dict(conv_padding="valid"), dict(conv_kernels=[[17, 41], [11, 21]]),
                                  dict(conv_kernels=[[11, 49], [11, 21]]), dict(conv_strides=[[4, 2], [1, 2]]),
                                  dict(conv_strides=[[2, 3], [1, 2]]), dict(conv_filters=[32, 40]), dict(conv_filters=[24, 32]),
                                  dict(conv_filters=[32, 144]), dict(rnn_units=500), dict(fc_units=1000)])
def test_options_that_are_not_built_fail_loudly(over):
    conf = dict(_fixture()["base"]["config"])
    conf.update(over)
    with pytest.raises(NotImplementedError, match=next(iter(over)).split("_")[0]):
        configs.deepspeech2_from_reference(conf)
    with pytest.raises(NotImplementedError):
        configs.deepspeech2(**over)


def test_options_the_reference_ignores_are_accepted():
    conf = dict(_fixture()["base"]["config"])
    conf.update(rnn_unroll=True, rnn_rowconv=3, rnn_rowconv_activation="tanh")  # bidirectional: RnnBlock builds no RowConv1D (:231)
    c = configs.deepspeech2_from_reference(conf)
    assert c.rnn_bidirectional and not c.has_rowconv
    assert not any("rowconv" in s[0] for s in params.param_specs(c))
    uni = dict(_fixture()["uni"]["config"])
    uni.update(rnn_rowconv_activation="tanh")
    with pytest.raises(NotImplementedError, match="rnn_rowconv_activation"):
        configs.deepspeech2_from_reference(uni)
    with pytest.raises(NotImplementedError, match="foo"):
        configs.deepspeech2_from_reference(dict(conf, foo=1))


@pytest.mark.parametrize("variant", ["base", "uni"])
def test_lengths(variant):
    """conv_output_length over the time stride (2, then 1): ceil(n / 2) under "same" and "causal"; the kernels' output sizes agree"""
    from tensorflowasr_amd.kernels import conv_pad_out

    c = configs.deepspeech2(variant=variant)
    assert [c.encoder_length(n) for n in (1, 2, 23, 1000)] == [1, 1, 12, 500]
    c3 = configs.DeepSpeech2Config(conv_padding=c.conv_padding)
    assert [c3.encoder_length(n) for n in (1, 2, 23, 1000)] == [1, 1, 8, 334]
    for T in (1, 2, 23, 1000):
        t = T
        for (kh, _), (st, _) in zip(c.conv_kernels, c.conv_strides):
            left, t = conv_pad_out(t, kh, st, c.conv_padding)
            assert left == kh - 1 or variant == "base"
        assert t == c.encoder_length(T)
    assert conv_pad_out(160, 41, 2, "same") == (19, 80) and conv_pad_out(160, 41, 2, "causal") == (40, 80)
    assert conv_pad_out(23, 11, 2, "same") == (5, 12) and conv_pad_out(1, 11, 2, "same") == (5, 1) and conv_pad_out(2, 11, 2, "same") == (4, 1)
    assert conv_pad_out(16, 6, 2, "same") == (2, 8) and conv_pad_out(7, 1, 2, "same") == (0, 4)


def test_parameter_names_under_the_references_layer_names():
    conv = lambda p: [p + "/kernel", p + "/bias"]
    bn = lambda p: [p + "/gamma", p + "/beta", p + "/moving_mean", p + "/moving_variance"]
    lstm = lambda p: [p + "/kernel", p + "/recurrent_kernel", p + "/bias"]
    for bi in (True, False):
        c = configs.deepspeech2_tiny(rnn_bidirectional=bi, rnn_rowconv=0 if bi else 2, conv_padding="same" if bi else "causal")
        want = []
        for i in range(2):
            want += conv(f"encoder/conv_module/block_{i}/conv2d") + bn(f"encoder/conv_module/block_{i}/bn")
        for i in range(2):
            p = f"encoder/rnn_module/block_{i}/"
            if bi:
                want += lstm(p + "blstm/forward_lstm") + lstm(p + "blstm/backward_lstm")
            else:
                want += lstm(p + "lstm") + [p + "rowconv/conv/kernel"] + bn(p + "rowconv/bn")
        want += conv("encoder/fc_module/block_0/fc") + conv("decoder/logits")
        names = [s[0] for s in params.param_specs(c)] + [b + leaf for b in params.bn_names(c) for leaf in ("/mm", "/mv")]
        got = [checkpoint.deepspeech2_keras_path(n) for n in names]
        assert sorted(got) == sorted(want) and len(set(got)) == len(got)
        shapes = {s[0]: s[1] for s in params.param_specs(c)}
        assert shapes["enc/conv_module/block_0/conv2d/w"] == (5, 7, 1, 16) and shapes["enc/conv_module/block_1/conv2d/w"] == (3, 5, 16, 16)
        first = "enc/rnn_module/block_0/" + ("blstm/forward_lstm" if bi else "lstm")
        second = "enc/rnn_module/block_1/" + ("blstm/backward_lstm" if bi else "lstm")
        assert shapes[first + "/k"] == (4 * 16, 128) and shapes[first + "/rk"] == (32, 128) and shapes[first + "/b"] == (128,)
        assert shapes[second + "/k"] == (64 if bi else 32, 128)
        assert shapes["enc/fc_module/block_0/fc/w"] == (64 if bi else 32, 64) and shapes["dec/logits/w"] == (64, 29)
        if not bi:
            assert shapes["enc/rnn_module/block_0/rowconv/conv/w"] == (5, 32)
    with pytest.raises(KeyError):
        checkpoint.deepspeech2_keras_path("pred/emb")


def test_spectrogram_band_table():
    from tensorflowasr_amd.deepspeech2 import spectrogram_weights

    for F in (16, 160, 257):
        melw, band = spectrogram_weights(F)
        assert melw.shape == (257, F) and melw.dtype == np.float32 and band.shape == (F, 2) and band.dtype == np.int32
        assert np.array_equal(melw[:F], np.eye(F, dtype=np.float32)) and not melw[F:].any()
        assert np.array_equal(band[:, 0], np.arange(F)) and np.array_equal(band[:, 1], np.arange(F))
        p = np.random.default_rng(F).random((3, 257)).astype(np.float32)
        assert np.array_equal(p @ melw, p[:, :F])  # the "mel" product is the first F power bins themselves


def test_model_registry_resolves_the_class_name(monkeypatch):
    from tensorflowasr_amd import base_model, deepspeech2

    seen = {}

    class Probe:
        def __init__(self, cfg, device, dtype=None, seed=0, dp=None):
            seen.update(cfg=cfg, seed=seed)

    monkeypatch.setattr(deepspeech2, "DeepSpeech2CTC", Probe)
    m = base_model.model_from_config(_fixture()["uni"], seed=7)
    assert isinstance(m, Probe) and seen["seed"] == 7 and isinstance(seen["cfg"], configs.DeepSpeech2Config) and seen["cfg"].has_rowconv


def test_abi_is_still_44_and_declares_the_new_symbols():
    hdr = open(os.path.join(HERE, "..", "include", "tfasr_hip.h")).read()
    assert re.search(r"#define\s+TFASR_ABI_VERSION\s+44\b", hdr) and _lib.ABI_VERSION == 44
    for name in ("tfasr_conv2d_fwd", "tfasr_conv2d_workspace_size", "tfasr_conv2d_pack_weight", "tfasr_conv2d_packed_weight_elems",
                 "tfasr_channel_affine_fwd", "tfasr_lstm_infer_fwd", "tfasr_lstm_infer_workspace_size"):
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["tfasr_conv2d_fwd"][1]) == 24 and len(_lib.SIGNATURES["tfasr_lstm_infer_fwd"][1]) == 16
    assert _lib.load(build_if_missing=False).tfasr_abi_version() == 44


def test_size_queries_answer_without_a_device():
    L = _lib.load(build_if_missing=False)
    n = ctypes.c_size_t(123)
    for dtype in (0, 1):
        assert L.tfasr_conv2d_workspace_size(32, 1000, 160, 500, 80, 1, 32, 11, 41, 2, 2, 5, 20, dtype, ctypes.byref(n)) == 0 and n.value == 0
        assert L.tfasr_lstm_infer_workspace_size(32, 500, 512, 2, dtype, ctypes.byref(n)) == 0
        # two 64-byte records, the per-step state; bf16 also the hand-off buffer [2, 32, 500, 512]
        assert n.value >= 128 + 32 * 2048 * 4 and (dtype == 0 or n.value >= 2 * 32 * 500 * 512 * 2)
    assert L.tfasr_conv2d_workspace_size(1, 8, 16, 8, 8, 16, 32, 3, 3, 1, 1, 1, 1, 0, None) == INVALID
    assert L.tfasr_conv2d_workspace_size(1, 8, 16, 2, 8, 16, 32, 3, 3, 4, 1, 1, 1, 0, ctypes.byref(n)) == UNSUPPORTED
    assert L.tfasr_lstm_infer_workspace_size(1, 8, 32, 2, 0, None) == INVALID
    assert L.tfasr_lstm_infer_workspace_size(1, 8, 32, 3, 0, ctypes.byref(n)) == INVALID
    assert L.tfasr_lstm_infer_workspace_size(0, 8, 32, 1, 0, ctypes.byref(n)) == INVALID
    assert L.tfasr_lstm_infer_workspace_size(65, 8, 48, 2, 1, ctypes.byref(n)) == 0  # outside the persistent range: still a legal shape
    e = ctypes.c_size_t(0)
    assert L.tfasr_conv2d_packed_weight_elems(11, 41, 1, 32, ctypes.byref(e)) == 0 and e.value == 11 * 64 * 32  # 41 taps padded to 2 k-steps
    assert L.tfasr_conv2d_packed_weight_elems(11, 21, 32, 32, ctypes.byref(e)) == 0 and e.value == 11 * 21 * 32 * 32
    assert L.tfasr_conv2d_packed_weight_elems(5, 7, 16, 48, ctypes.byref(e)) == 0 and e.value == 5 * 4 * 64 * 32
    assert L.tfasr_conv2d_packed_weight_elems(17, 7, 16, 48, ctypes.byref(e)) == UNSUPPORTED
    assert L.tfasr_conv2d_packed_weight_elems(5, 7, 16, 48, None) == INVALID
    ptr = ctypes.c_void_p(4096)
    assert L.tfasr_conv2d_pack_weight(None, ptr, 5, 7, 16, 48, None) == INVALID
    assert L.tfasr_conv2d_pack_weight(ptr, ptr, 5, 49, 16, 48, None) == UNSUPPORTED
    assert L.tfasr_conv2d_pack_weight(ptr, ptr, 5, 7, 16, 0, None) == INVALID


@pytest.mark.parametrize("over,want", [(dict(x=None), INVALID), (dict(w=None), INVALID), (dict(y=None), INVALID), (dict(B=0), INVALID),
                                       (dict(T=0), INVALID), (dict(F=-1), INVALID), (dict(To=0), INVALID), (dict(Fo=0), INVALID),
                                       (dict(kh=0), INVALID), (dict(kw=0), INVALID), (dict(st=0), INVALID), (dict(sf=0), INVALID),
                                       (dict(Cin=0), INVALID), (dict(Cout=0), INVALID), (dict(pad_t=-1), INVALID), (dict(dtype=2), INVALID),
                                       (dict(x=ctypes.c_void_p(4100)), INVALID),
                                       (dict(kh=17), UNSUPPORTED), (dict(kw=49), UNSUPPORTED), (dict(st=4), UNSUPPORTED),
                                       (dict(sf=3), UNSUPPORTED), (dict(Cin=24), UNSUPPORTED), (dict(Cin=2), UNSUPPORTED),
                                       (dict(Cout=40), UNSUPPORTED), (dict(Cout=144), UNSUPPORTED)])
def test_conv2d_fwd_rejects_bad_arguments_before_any_launch(over, want):
    """no device is needed (or touched): the pointers are never dereferenced"""
    L = _lib.load(build_if_missing=False)
    ptr = ctypes.c_void_p(4096)
    a = dict(x=ptr, w=ptr, y=ptr, B=1, T=8, F=16, To=4, Fo=8, Cin=16, Cout=32, kh=5, kw=7, st=2, sf=2, pad_t=2, pad_f=3, dtype=0)
    a.update(over)
    for dtype in ((0, 1) if "dtype" not in over else (over["dtype"],)):
        st = L.tfasr_conv2d_fwd(a["x"], a["w"], None, None, None, a["y"], a["B"], a["T"], a["F"], a["To"], a["Fo"], a["Cin"], a["Cout"], a["kh"],
                                a["kw"], a["st"], a["sf"], a["pad_t"], a["pad_f"], 0, dtype, None, 0, None)
        assert st == want


@pytest.mark.parametrize("over", [dict(xg=None), dict(rk=None), dict(y=None), dict(ws=None), dict(B=0), dict(T=0), dict(P=0), dict(ndir=0),
                                  dict(ndir=3), dict(dtype=2), dict(ld_xg=255), dict(ld_y=63), dict(ld_xg=257), dict(ws_bytes=64),
                                  dict(xg=ctypes.c_void_p(4098)), dict(ws=ctypes.c_void_p(4100))])
def test_lstm_infer_fwd_rejects_bad_arguments_before_any_launch(over):
    L = _lib.load(build_if_missing=False)
    ptr = ctypes.c_void_p(4096)
    a = dict(xg=ptr, rk=ptr, y=ptr, ws=ptr, B=2, T=4, P=32, ndir=2, dtype=1, ld_xg=256, ld_y=64, ws_bytes=1 << 30)
    a.update(over)
    st = L.tfasr_lstm_infer_fwd(a["xg"], a["ld_xg"], a["rk"], None, a["y"], a["ld_y"], None, None, a["B"], a["T"], a["P"], a["ndir"], a["dtype"],
                                a["ws"], a["ws_bytes"], None)
    assert st == INVALID


def test_channel_affine_rejects_bad_arguments():
    L = _lib.load(build_if_missing=False)
    ptr = ctypes.c_void_p(4096)
    assert L.tfasr_channel_affine_fwd(None, None, None, ptr, 4, 16, 1, 0, None) == INVALID
    assert L.tfasr_channel_affine_fwd(ptr, None, None, ptr, 0, 16, 1, 0, None) == INVALID
    assert L.tfasr_channel_affine_fwd(ptr, None, None, ptr, 4, 16, 1, 2, None) == INVALID
