"""Jasper CTC without a device: the config surface against the rendered reference YAML (tests/golden/jasper_config.json, made by
tools/render_jasper_config.py), lengths, the parameter set under the reference's layer names, and the Conv1D entry points' host-side
argument checks (csrc/conv1d.hip)."""
import ctypes
import dataclasses
import json
import os
import re

import pytest

from tensorflowasr_amd import _lib, checkpoint, configs, params

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture():
    with open(os.path.join(HERE, "golden", "jasper_config.json")) as f:
        return json.load(f)


def test_reference_yaml_equals_the_shipped_config_field_by_field():
    fx = _fixture()
    assert fx["class_name"] == "tensorflow_asr.models.ctc.jasper>Jasper"
    got, want = configs.jasper_from_reference(fx["config"]), configs.jasper(vocab_size=1000)
    for f in dataclasses.fields(configs.JasperConfig):
        assert getattr(got, f.name) == getattr(want, f.name), f.name
    assert got.log_base == "10" and got.dense and got.nsubblocks == 3 and got.block_kernels == [11, 13, 17, 21, 25]


def test_log_base_10_is_jaspers_alone():
    sc = _fixture()["config"]["speech_config"]
    assert sc["log_base"] == "10"
    with pytest.raises(NotImplementedError):
        configs.ConformerConfig.from_reference({"speech_config": sc})
    with pytest.raises(NotImplementedError):
        configs.speech_kwargs(sc)
    assert configs.speech_kwargs(sc, log_bases=("e", "10"))["num_feature_bins"] == 80


def test_10x5_layout():
    c = configs.jasper(layout="10x5")
    assert c.nsubblocks == 5 and c.dense
    assert c.block_channels == [256, 256, 384, 384, 512, 512, 640, 640, 768, 768]
    assert c.block_kernels == [11, 11, 13, 13, 17, 17, 21, 21, 25, 25]


@pytest.mark.parametrize("over", [dict(padding="same"), dict(first_additional_block_strides=4), dict(second_additional_block_strides=2),
                                  dict(third_additional_block_strides=2), dict(block_channels=[256, 392, 512, 640, 768]),
                                  dict(first_additional_block_channels=250), dict(block_kernels=[11, 13, 17, 21, 33])])
def test_options_that_are_not_built_fail_loudly(over):
    conf = dict(_fixture()["config"])
    conf.update(over)
    with pytest.raises(NotImplementedError):
        configs.jasper_from_reference(conf)
    with pytest.raises(NotImplementedError):
        configs.jasper(**over)


def test_time_reduction_and_lengths():
    c = configs.jasper()
    assert c.time_reduction_factor == 2
    assert [c.encoder_length(n) for n in (0, 1, 2, 7, 8)] == [0, 1, 1, 4, 4]
    assert configs.jasper(first_additional_block_strides=1).time_reduction_factor == 1


def test_parameter_names_of_a_dense_two_block_config():
    c = configs.jasper_tiny(nsubblocks=3, block_channels=[64, 96], block_kernels=[11, 13], block_dropout=[0.0, 0.0])
    conv = lambda p: [p + "/kernel", p + "/bias"]
    bn = lambda p: [p + "/gamma", p + "/beta", p + "/moving_mean", p + "/moving_variance"]
    sub = lambda p: conv(p + "/conv1d") + bn(p + "/bn")
    res = lambda p: conv(p + "/pointwise_conv1d") + bn(p + "/bn")
    want = sub("encoder/first_block")
    for i in range(2):
        for j in range(3):
            want += sub(f"encoder/block_{i}/subordinate_{j}")
        for r in range(i + 1):  # dense: block i's last sub-block has i + 1 residual branches
            want += res(f"encoder/block_{i}/subordinate_2/residual_{r}")
    want += sub("encoder/second_block") + sub("encoder/third_block") + conv("decoder/logits")
    names = [s[0] for s in params.param_specs(c)] + [b + leaf for b in params.bn_names(c) for leaf in ("/mm", "/mv")]
    got = [checkpoint.jasper_keras_path(n) for n in names]
    assert sorted(got) == sorted(want) and len(set(got)) == len(got)
    shapes = {s[0]: s[1] for s in params.param_specs(c)}
    assert shapes["enc/first_block/conv1d/w"] == (11, 80, 48) and shapes["enc/block_1/subordinate_0/conv1d/w"] == (13, 64, 96)
    assert shapes["enc/block_1/subordinate_2/residual_0/pointwise_conv1d/w"] == (1, 48, 96)  # the first block's output feeds block 0
    assert shapes["enc/block_1/subordinate_2/residual_1/pointwise_conv1d/w"] == (1, 64, 96)
    assert shapes["dec/logits/w"] == (160, 29)
    # not dense: one branch per block, fed by the block's own input
    nd = [s[0] for s in params.param_specs(configs.jasper_tiny(dense=False))]
    assert sum("residual_1" in n for n in nd) == 0 and sum("block_1/subordinate_2/residual_0" in n for n in nd) == 4


def test_abi_is_still_44_and_declares_the_conv1d_symbols():
    hdr = open(os.path.join(HERE, "..", "include", "tfasr_hip.h")).read()
    assert re.search(r"#define\s+TFASR_ABI_VERSION\s+44\b", hdr) and _lib.ABI_VERSION == 44
    for name in ("tfasr_conv1d_fwd", "tfasr_conv1d_workspace_size", "tfasr_conv1d_pack_weight", "tfasr_conv1d_packed_weight_elems",
                 "tfasr_conv1d_tail_update"):
        assert name in _lib.SIGNATURES, name
    assert _lib.load(build_if_missing=False).tfasr_abi_version() == 44


def test_workspace_size_answers_without_a_device():
    L = _lib.load(build_if_missing=False)
    n = ctypes.c_size_t(123)
    for dtype in (0, 1):
        assert L.tfasr_conv1d_workspace_size(32, 1000, 80, 256, 11, 2, 1, dtype, ctypes.byref(n)) == 0
        assert n.value < (1 << 30)
    assert L.tfasr_conv1d_workspace_size(1, 8, 80, 256, 11, 3, 1, 0, ctypes.byref(n)) == _lib.STATUS_UNSUPPORTED
    assert L.tfasr_conv1d_workspace_size(1, 8, 80, 256, 11, 1, 1, 0, None) == 1
    e = ctypes.c_size_t(0)
    assert L.tfasr_conv1d_packed_weight_elems(11, 80, 256, ctypes.byref(e)) == 0 and e.value >= 11 * 80 * 256


@pytest.mark.parametrize("over,want", [(dict(x=None), (1,)), (dict(w=None), (1,)), (dict(y=None), (1,)), (dict(K=0), (1, 3)), (dict(K=33), (1, 3)),
                                       (dict(stride=3), (1, 3)), (dict(Cin=24), (1, 3)), (dict(Cout=40), (1, 3)), (dict(dilation=0), (1, 3)),
                                       (dict(K=32, dilation=9), (3,)), (dict(dtype=2), (1,)), (dict(x=ctypes.c_void_p(4100)), (1,))])
def test_conv1d_fwd_rejects_bad_arguments_before_any_launch(over, want):
    """no device is needed (or touched): the pointers are never dereferenced"""
    L = _lib.load(build_if_missing=False)
    ptr = ctypes.c_void_p(4096)
    a = dict(x=ptr, w=ptr, y=ptr, B=1, T=8, lead=0, Cin=80, Cout=64, K=11, stride=1, dilation=1, dtype=0)
    a.update(over)
    st = L.tfasr_conv1d_fwd(a["x"], a["w"], None, None, None, None, a["y"], a["B"], a["T"], a["lead"], a["Cin"], a["Cout"], a["K"], a["stride"],
                            a["dilation"], 0, a["dtype"], None, 0, None)
    assert st in want


def test_an_empty_problem_is_a_success_that_launches_nothing():
    L = _lib.load(build_if_missing=False)
    ptr = ctypes.c_void_p(4096)
    for B, T in ((0, 8), (3, 0)):
        assert L.tfasr_conv1d_fwd(ptr, ptr, None, None, None, None, ptr, B, T, 0, 80, 64, 11, 1, 1, 0, 0, None, 0, None) == 0


def test_model_registry_still_refuses_the_class_name():
    from tensorflowasr_amd.base_model import model_from_config

    with pytest.raises(NotImplementedError):
        model_from_config(_fixture())
