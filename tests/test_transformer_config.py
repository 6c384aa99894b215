"""TransformerConfig and its constructors against the reference's shipped YAMLs (tests/golden/transformer_config.json), the options that
are not built, the parameter table under the reference's names, and the C ABI of the plain-attention kernel - all without a GPU."""
import ctypes
import dataclasses
import json
import os
import re

import numpy as np
import pytest
import torch

from tensorflowasr_amd import _lib, base_model, checkpoint, configs
from tensorflowasr_amd.params import ParamStore, param_specs, transformer_modules

import transformer_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 3


def _fixture():
    with open(C.CONFIG_FIXTURE) as f:
        return json.load(f)


@pytest.mark.skipif(not C.have_reference(), reason="the reference tree is not on this machine")
def test_fixture_equals_a_fresh_rendering():
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_transformer_fixtures as G
    finally:
        sys.path.pop(0)
    assert G.render_configs() == _fixture()


@pytest.mark.parametrize("key,streaming", [("base", False), ("base-streaming", True)])
def test_reference_yaml_equals_the_shipped_config_field_by_field(key, streaming):
    fx = _fixture()[key]
    assert fx["class_name"] == "tensorflow_asr.models.ctc.transformer>Transformer" and fx["config"]["vocab_size"] == 1000
    got = configs.transformer_from_reference(fx["config"], class_name=fx["class_name"])
    want = configs.transformer(vocab_size=1000, streaming=streaming)
    for f in dataclasses.fields(configs.TransformerConfig):
        assert getattr(got, f.name) == getattr(want, f.name), f.name
    assert (got.chunk_size, got.history_size) == ((16, 64) if streaming else (None, None))
    assert got.encoder == "transformer" and got.head == "ctc" and got.dmodel == 512 and got.head_size == 128 and got.mha_type == "mha"
    assert got.encoder_length(1000) == 250 and got.sub_freq == 20 and got.time_reduction_factor == 4
    # the same mapping under the transducer class
    t = configs.transformer_from_reference(dict(fx["config"], prediction_rnn_units=64, joint_dim=48), head="rnnt")
    assert t.head == "transducer" and t.rnn_units == 64 and t.joint_dim == 48 and t.embed_dim == 512
    assert configs.transformer(head="rnnt").head == "transducer"


@pytest.mark.parametrize("over,name", [
    (dict(encoder_mha_type="relmha"), "encoder_mha_type"), (dict(encoder_memory_length=8), "encoder_memory_length"),
    (dict(encoder_norm_position="none"), "encoder_norm_position"), (dict(encoder_pwffn_activation="gelu"), "encoder_pwffn_activation"),
    (dict(encoder_head_size=96 + 8), "encoder_head_size"), (dict(encoder_head_size=256), "encoder_head_size"),
    (dict(encoder_dmodel=100), "encoder_dmodel"), (dict(encoder_trainable=False), "encoder_trainable"),
    (dict(decoder_trainable=False), "decoder_trainable"), (dict(bias_regularizer={"class_name": "l2"}), "bias_regularizer"),
    (dict(kernel_regularizer={"class_name": "l1"}), "kernel_regularizer"), (dict(prediction_embed_dim=8), "prediction_embed_dim"),
    (dict(encoder_kernel_size=31), "encoder_kernel_size"), (dict(unknown_option=1), "unknown_option")])
def test_options_that_are_not_built_raise_by_name(over, name):
    conf = dict(_fixture()["base"]["config"])
    conf.update(over)
    with pytest.raises(NotImplementedError, match=name):
        configs.transformer_from_reference(conf)


@pytest.mark.parametrize("sub,name", [(dict(type="vgg"), "type"), (dict(type="conv1d"), "type"), (dict(kernels=[5, 5]), "kernels"),
                                      (dict(strides=[2, 1]), "strides"), (dict(paddings=["same", "same"]), "paddings"),
                                      (dict(norms=["layer", "layer"]), "norms"), (dict(norms=["batch", "none"]), "norms"),
                                      (dict(activations=["swish", "swish"]), "activations"), (dict(filters=[12, 12]), "filters"),
                                      (dict(filters=[16, 16, 16]), "filters"), (dict(dilations=[1, 1]), "dilations")])
def test_subsampling_options_that_are_not_built_raise_by_name(sub, name):
    conf = dict(_fixture()["base"]["config"])
    conf["encoder_subsampling"] = dict(conf["encoder_subsampling"], **sub)
    with pytest.raises(NotImplementedError, match=name):
        configs.transformer_from_reference(conf)


def test_defaults_omitted_from_the_mapping_are_the_classes():
    """the classes default to relmha and to strides [[2, 1], [2, 1]]: a mapping that leaves them out is not the shipped network"""
    conf = dict(_fixture()["base"]["config"])
    del conf["encoder_mha_type"]
    with pytest.raises(NotImplementedError, match="encoder_mha_type"):
        configs.transformer_from_reference(conf)
    conf = dict(_fixture()["base"]["config"])
    conf["encoder_subsampling"] = {k: v for k, v in conf["encoder_subsampling"].items() if k != "strides"}
    with pytest.raises(NotImplementedError, match="strides"):
        configs.transformer_from_reference(conf)
    # accepted: options that change nothing in the mha encoder's inference arithmetic, both norms, pre-norm, the causal flag, one-sided window
    conf = dict(_fixture()["base"]["config"], encoder_mha_causal=True, encoder_flash_attention=True, encoder_norm_position="pre",
                encoder_use_attention_causal_mask=True, encoder_interleave_relpe=False, encoder_chunk_size=8)
    conf["encoder_subsampling"] = dict(conf["encoder_subsampling"], norms=["none", "none"])
    c = configs.transformer_from_reference(conf)
    assert (c.norm_position, c.use_attention_causal_mask, c.interleave_relpe, c.sub_norm) == ("pre", True, False, "none")
    assert c.chunk_size is None and c.history_size is None  # the streaming mask needs both (multihead_attention.py:342)


def test_conformer_keeps_refusing_mha_and_the_registry_knows_the_transformers():
    with pytest.raises(NotImplementedError):
        configs.ConformerConfig.from_reference({"encoder_mha_type": "mha"})
    with pytest.raises(NotImplementedError):
        base_model.model_from_config({"class_name": "tensorflow_asr.models.ctc.jasper>Jasper", "config": {}})
    # the Transformer class names resolve: what stops them here is the missing device, not the registry
    if not torch.cuda.is_available():
        for cls in ("ctc", "transducer"):
            with pytest.raises(_lib.TfasrError, match="MI355X"):
                base_model.model_from_config({"class_name": f"tensorflow_asr.models.{cls}.transformer>Transformer", "config": _fixture()["base"]["config"]})


def test_parameter_names_and_shapes():
    cfg = C.tiny_config("full")
    specs = {n: s for n, s, *_ in param_specs(cfg)}
    assert specs["enc/subsampling/block_0/conv_0/w"] == (3, 3, 1, 16) and specs["enc/subsampling/block_1/conv_1/w"] == (3, 3, 16, 16)
    assert specs["enc/linear/w"] == (4 * 16, 64) and specs["enc/block_1/mhsa/qkv/w"] == (64, 3 * 2 * 64) and specs["enc/block_1/mhsa/o/w"] == (128, 64)
    assert specs["enc/block_0/pwffn/ffn_1/w"] == (64, 128) and specs["enc/block_0/pwffn/ffn_2/w"] == (128, 64) and specs["dec/logits/w"] == (64, 29)
    assert transformer_modules(cfg)["blocks"] == ["enc/block_0", "enc/block_1"]
    ps = ParamStore(cfg, torch.device("cpu"), torch.float32, 1)
    assert sorted(ps.state) == sorted(f"enc/subsampling/block_{i}/bn_{i}/{s}" for i in (0, 1) for s in ("mm", "mv"))
    W = ps.export_keras()
    arrays = checkpoint.to_keras(W, path_fn=checkpoint.transformer_keras_path)
    want = {"encoder/subsampling/block_0/conv_0/kernel": (3, 3, 1, 16), "encoder/subsampling/block_1/bn_1/moving_variance": (16,),
            "encoder/subsampling/block_0/bn_0/beta": (16,), "encoder/linear/kernel": (64, 64), "encoder/block_0/mhsa/query/kernel": (64, 2, 64),
            "encoder/block_1/mhsa/key/bias": (2, 64), "encoder/block_1/mhsa/value/kernel": (64, 2, 64),
            "encoder/block_0/mhsa/attention_output/kernel": (2, 64, 64), "encoder/block_0/mhsa/attention_output/bias": (64,),
            "encoder/block_1/ln_1/gamma": (64,), "encoder/block_1/ln_2/beta": (64,), "encoder/block_0/pwffn/ffn_1/kernel": (64, 128),
            "encoder/block_0/pwffn/ffn_2/bias": (64,), "decoder/logits/kernel": (64, 29), "decoder/logits/bias": (29,)}
    for path, shape in want.items():
        assert arrays[path].shape == shape, path
    assert len(arrays) == 12 + 2 + 2 * 16 + 2
    # fused <-> Keras layouts, both ways: the query kernel is the first H dh columns of the fused matrix, head-major
    qkv = ps.p("enc/block_0/mhsa/qkv/w")
    assert np.array_equal(arrays["encoder/block_0/mhsa/key/kernel"], qkv[:, 128:256].reshape(64, 2, 64).numpy())
    back = checkpoint.from_keras(arrays, W, path_fn=checkpoint.transformer_keras_path)
    ps2 = ParamStore(cfg, torch.device("cpu"), torch.float32, 2)
    ps2.import_keras({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in back.items()})
    assert torch.equal(ps2.flat, ps.flat)
    # the transducer keeps the Conformer transducer's prediction / joint names; no BatchNorm state without a norm
    t = ParamStore(C.tiny_config("full", head="rnnt", sub_norm="none"), torch.device("cpu"), torch.float32, 1)
    paths = checkpoint.to_keras(t.export_keras(), path_fn=checkpoint.transformer_keras_path)
    assert "prediction/lstm_0/lstm_cell/recurrent_kernel" in paths and "joint/vocab/kernel" in paths and "decoder/logits/kernel" not in paths
    assert not t.state and not any("bn_" in p for p in paths)


def test_abi_is_still_44_and_declares_the_new_symbols():
    hdr = open(os.path.join(ROOT, "include", "tfasr_hip.h")).read()
    assert re.search(r"#define\s+TFASR_ABI_VERSION\s+44\b", hdr) and _lib.ABI_VERSION == 44
    for name, nargs in (("tfasr_attn_plain_fwd", 15), ("tfasr_add_pe", 9)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
    L = _lib.load(build_if_missing=False)
    assert L.tfasr_abi_version() == 44 and hasattr(L, "tfasr_attn_plain_fwd") and hasattr(L, "tfasr_add_pe")


@pytest.mark.parametrize("over,dtypes,want", [
    (dict(qkv=None), (0, 1), INVALID), (dict(out=None), (0, 1), INVALID), (dict(B=0), (0, 1), INVALID), (dict(T=0), (0, 1), INVALID),
    (dict(H=0), (0, 1), INVALID), (dict(dh=0), (0, 1), INVALID), (dict(lengths=None), (0, 1), INVALID), (dict(), (2,), INVALID),
    (dict(qkv=ctypes.c_void_p(4100)), (1,), INVALID),
    (dict(dh=96), (1,), UNSUPPORTED), (dict(dh=32), (1,), UNSUPPORTED), (dict(dh=256), (0, 1), UNSUPPORTED), (dict(dh=24), (0,), UNSUPPORTED),
    (dict(dh=144), (0,), UNSUPPORTED), (dict(B=70000), (0, 1), UNSUPPORTED)])
def test_attn_plain_fwd_rejects_bad_arguments_before_any_launch(over, dtypes, want):
    """no device is needed (or touched): the pointers are never dereferenced"""
    L = _lib.load(build_if_missing=False)
    ptr = ctypes.c_void_p(4096)
    a = dict(qkv=ptr, lengths=ptr, out=ptr, B=2, H=2, T=8, dh=64)
    a.update(over)
    for dtype in dtypes:
        st = L.tfasr_attn_plain_fwd(a["qkv"], a["lengths"], a["out"], None, a["B"], a["H"], a["T"], a["dh"], 0.125, 1, 0, 0, 0, dtype, None)
        assert st == want, dtype


def test_add_pe_rejects_bad_arguments():
    L = _lib.load(build_if_missing=False)
    ptr = ctypes.c_void_p(4096)
    assert L.tfasr_add_pe(None, ptr, None, ptr, 1, 4, 16, 0, None) == INVALID
    assert L.tfasr_add_pe(ptr, None, None, ptr, 1, 4, 16, 0, None) == INVALID
    assert L.tfasr_add_pe(ptr, ptr, None, ptr, 1, 4, 12, 0, None) == INVALID
    assert L.tfasr_add_pe(ptr, ptr, None, ptr, 0, 4, 16, 1, None) == INVALID
    assert L.tfasr_add_pe(ptr, ptr, None, ptr, 1, 4, 16, 2, None) == INVALID
