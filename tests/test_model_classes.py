"""The class structure of the models (model.AsrModel's docstring): an encoder mixin in front of a head, over AsrModel.  Classes only: no
GPU, no model instance."""
import inspect
import os
import re

import pytest

import tensorflowasr_amd
from tensorflowasr_amd.conformer import ConformerEncoderMixin, ConformerTransducer
from tensorflowasr_amd.contextnet import ContextNetEncoderMixin, ContextNetTransducer
from tensorflowasr_amd.ctc_model import ConformerCTC, CtcModel
from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC, DeepSpeech2EncoderMixin
from tensorflowasr_amd.inference_only import InferenceOnlyEncoder
from tensorflowasr_amd.jasper import JasperCTC, JasperEncoderMixin
from tensorflowasr_amd.model import AsrModel
from tensorflowasr_amd.rnnt import RnnEncoderMixin, RnnTransducer
from tensorflowasr_amd.transducer import TransducerModel
from tensorflowasr_amd.transformer import TransformerCTC, TransformerEncoderMixin, TransformerTransducer

PKG = os.path.dirname(os.path.abspath(tensorflowasr_amd.__file__))
# class -> (encoder mixin, head)
TABLE = {
    ConformerTransducer: (ConformerEncoderMixin, TransducerModel),
    ConformerCTC: (ConformerEncoderMixin, CtcModel),
    ContextNetTransducer: (ContextNetEncoderMixin, TransducerModel),
    TransformerTransducer: (TransformerEncoderMixin, TransducerModel),
    TransformerCTC: (TransformerEncoderMixin, CtcModel),
    RnnTransducer: (RnnEncoderMixin, TransducerModel),
    JasperCTC: (JasperEncoderMixin, CtcModel),
    DeepSpeech2CTC: (DeepSpeech2EncoderMixin, CtcModel),
}
INFERENCE_ONLY = (TransformerTransducer, TransformerCTC, RnnTransducer, JasperCTC, DeepSpeech2CTC)
CTC = [c for c, (_, head) in TABLE.items() if head is CtcModel]


def _package_sources():
    for name in sorted(os.listdir(PKG)):
        if name.endswith(".py"):
            with open(os.path.join(PKG, name)) as f:
                yield name, f.read()


@pytest.mark.parametrize("cls", list(TABLE), ids=lambda c: c.__name__)
def test_mro_is_encoder_then_head_then_base(cls):
    enc, head = TABLE[cls]
    assert cls.__bases__ == (enc, head)
    mro = [k for k in cls.__mro__ if k not in (cls, InferenceOnlyEncoder, object)]
    assert mro == [enc, head, AsrModel, tensorflowasr_amd.base_model.BaseModel]
    assert (InferenceOnlyEncoder in cls.__mro__) == (cls in INFERENCE_ONLY)
    if cls in INFERENCE_ONLY:  # the refusals of the training entry points come before the head's methods
        assert cls.__mro__.index(InferenceOnlyEncoder) == 2
    assert (ConformerEncoderMixin in cls.__mro__) == (cls in (ConformerTransducer, ConformerCTC))
    assert cls.encoder_kind == vars(enc)["encoder_kind"] and cls.head_kind == vars(head)["head_kind"]
    assert "__init__" not in vars(cls) and "__init__" not in vars(enc) and "__init__" not in vars(head)
    assert cls.__init__ is AsrModel.__init__


@pytest.mark.parametrize("cls", CTC, ids=lambda c: c.__name__)
def test_ctc_classes_hold_no_transducer_code(cls):
    for name in ("prediction_fwd", "joint_fwd", "_greedy_search"):
        assert not hasattr(cls, name)
    m = object.__new__(cls)
    for name, word in (("align_encoded", "lattice"), ("recognize_encoded", "greedy search"), ("recognize_encoded_detailed", "greedy search"),
                       ("recognize_beam_encoded", "beam search")):
        assert vars(CtcModel)[name] is getattr(cls, name)
        with pytest.raises(NotImplementedError, match=word + ".*CTC model"):
            getattr(m, name)(None, None)


def test_native_blocks_is_assigned_in_one_place():
    hits = [(name, line.strip()) for name, src in _package_sources() for line in src.splitlines() if re.search(r"\bnative_blocks\s*=[^=]", line)]
    assert len(hits) == 1 and hits[0][0] == "conformer.py", hits


@pytest.mark.parametrize("name", ["_cache", "_affine", "_inference_only"])
def test_inference_only_boilerplate_has_one_copy(name):
    defs = [fname for fname, src in _package_sources() if re.search(rf"^\s*def {name}\(", src, re.M)]
    assert defs == ["inference_only.py"], defs
    want = os.path.join(PKG, "inference_only.py")
    for cls in INFERENCE_ONLY:
        fn = getattr(cls, name)
        assert fn is vars(InferenceOnlyEncoder)[name]
        assert fn.__qualname__ == "InferenceOnlyEncoder." + name and os.path.samefile(inspect.getsourcefile(fn), want)
    for cls in set(TABLE) - set(INFERENCE_ONLY):
        assert not hasattr(cls, name)


def test_inference_only_messages_keep_each_models_sentence():
    for cls, words in ((JasperCTC, "JasperCTC is inference only: the Conv1D data / weight gradients"),
                       (DeepSpeech2CTC, "DeepSpeech2CTC is inference only: the Conv2D / LSTM gradients"),
                       (TransformerCTC, "TransformerCTC is inference only: the plain-attention backward"),
                       (TransformerTransducer, "TransformerTransducer is inference only: the plain-attention backward"),
                       (RnnTransducer, "RnnTransducer is inference only: the encoder's LSTM and block-tail gradients")):
        m = object.__new__(cls)
        for entry in ("train_step", "loss_and_backward", "compile"):
            assert getattr(cls, entry) is InferenceOnlyEncoder._inference_only
            with pytest.raises(NotImplementedError, match=re.escape(words) + r".* are not built \(weights arrive through load_weights\)"):
                getattr(m, entry)()
        with pytest.raises(NotImplementedError, match="inference only"):
            m.frontend(None, None, training=True)


def test_config_of_another_model_is_refused_before_the_device_is_touched():
    from tensorflowasr_amd import configs

    for cls, bad in ((ConformerTransducer, configs.conformer_ctc_s()), (ConformerCTC, configs.conformer_tiny()), (JasperCTC, configs.conformer_ctc_s()),
                     (DeepSpeech2CTC, configs.jasper_tiny()), (TransformerCTC, configs.transformer_tiny(head="rnnt")),
                     (TransformerTransducer, configs.transformer_tiny()), (RnnTransducer, configs.transformer_tiny(head="rnnt")),
                     (ContextNetTransducer, configs.conformer_tiny())):
        with pytest.raises(ValueError, match=cls.__name__ + " needs a"):
            cls(bad)
