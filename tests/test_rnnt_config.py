"""RnnTransducerConfig: the rendered small.yml.j2 (tests/golden/rnnt_config.json) round-trips through rnnt_from_reference, every option
that is not built raises with its name, model_from_config resolves the reference's class name, and the checkpoint paths are the
reference's layer names.  CPU only."""
import json

import pytest
import torch

from tensorflowasr_amd import base_model, checkpoint, configs
from tensorflowasr_amd.params import ParamStore, rnnt_modules

import rnnt_cases as C

CLASS = "tensorflow_asr.models.transducer.rnnt>RnnTransducer"


@pytest.fixture(scope="module")
def fixture():
    with open(C.CONFIG_FIXTURE) as f:
        return json.load(f)


def test_fixture_round_trips(fixture):
    assert fixture["class_name"] == CLASS
    cfg = configs.rnnt_from_reference(fixture["config"])
    want = configs.rnnt(vocab_size=1000)
    assert cfg == want
    assert (cfg.reduction_positions, cfg.reduction_factors, cfg.nlayers) == (["post"] * 4, [3, 0, 2, 0], 4)
    assert (cfg.encoder_dmodel, cfg.dmodel, cfg.encoder_rnn_units, cfg.layer_norm) == (320, 320, 1024, True)
    assert (cfg.embed_dim, cfg.rnn_units, cfg.joint_dim, cfg.prediction_layer_norm, cfg.vocab_size, cfg.blank) == (512, 1024, 320, True, 1000, 0)
    assert cfg.l2 == 1e-6 and cfg.num_feature_bins == 80 and cfg.time_masking["num_masks"] == 5 and cfg.freq_masking["mask_factor"] == 27
    assert cfg.time_reduction_factor == 6 and cfg.encoder_length(1000) == 167 and cfg.head == "transducer" and cfg.encoder == "rnnt"
    assert [(m["din"], m["P"], m["dout"], m["factor"]) for m in rnnt_modules(cfg)] == [(80, 1024, 320, 3), (960, 1024, 320, 1), (320, 1024, 320, 2),
                                                                                        (640, 1024, 320, 1)]


def test_every_keyword_of_the_class_is_taken_or_refused_by_name(fixture):
    base = fixture["config"]
    ok = dict(encoder_reduction_positions=["pre", "post", "pre", "post"], encoder_reduction_factors=[2, 2, 0, 3], encoder_dmodel=64,
              encoder_rnn_units=96, encoder_layer_norm=False, encoder_rnn_unroll=True, prediction_rnn_implementation=1,
              prediction_rnn_unroll=True, prediction_embed_dim=8, prediction_rnn_units=16, joint_dim=24, blank=0, name="x")
    cfg = configs.rnnt_from_reference(dict(base, **ok))
    assert cfg.time_reduction_factor == 12 and cfg.dmodel == 192 and not cfg.layer_norm  # a `post` reduction in the last block widens the rows
    assert [cfg.lstm_in(i) for i in range(4)] == [160, 64, 128, 64]
    refused = dict(encoder_rnn_type="gru", prediction_num_rnns=2, prediction_projection_units=640, prediction_rnn_type="gru",
                   prediction_layer_norm=False, prediction_label_encode_mode="one_hot", joint_activation="relu", joint_mode="concat",
                   prejoint_encoder_linear=False, prejoint_prediction_linear=False, postjoint_linear=True, encoder_trainable=False,
                   prediction_trainable=False, joint_trainable=False, bias_regularizer={"class_name": "l2", "config": {"l2": 1e-6}},
                   activity_regularizer="l2", encoder_rnn_units=100, encoder_dmodel=24, something_else=1)
    for k, v in refused.items():
        with pytest.raises(NotImplementedError, match=k):
            configs.rnnt_from_reference(dict(base, **{k: v}))
    with pytest.raises(NotImplementedError, match="encoder_rnn_type"):
        configs.rnnt_from_reference(dict(base, encoder_rnn_type="rnn"))
    with pytest.raises(NotImplementedError, match="kernel_regularizer"):
        configs.rnnt_from_reference(dict(base, kernel_regularizer={"class_name": "l1", "config": {}}))
    with pytest.raises(NotImplementedError, match="feature_type"):
        configs.rnnt_from_reference(dict(base, speech_config=dict(base["speech_config"], feature_type="mfcc")))
    # a keyword the mapping omits takes the CLASS's default: two prediction LSTMs with a projection, which is not built
    with pytest.raises(NotImplementedError, match="prediction_num_rnns"):
        configs.rnnt_from_reference({k: v for k, v in base.items() if k != "prediction_num_rnns"})
    small = {k: v for k, v in base.items() if not k.startswith("encoder_")}
    assert configs.rnnt_from_reference(small).reduction_factors == [6, 0, 0, 0, 0, 0, 0, 0]
    for bad in (dict(encoder_reduction_positions=["post"] * 3), dict(encoder_reduction_factors=[1, 2]), dict(encoder_reduction_positions=["mid"] * 4),
                dict(encoder_reduction_factors=[3, -1, 0, 0]), dict(encoder_nlayers=0)):
        with pytest.raises(ValueError):
            configs.rnnt_from_reference(dict(base, **bad))


def test_class_name_resolves(fixture, monkeypatch):
    seen = {}

    class Fake:
        def __init__(self, cfg, device=None, dtype=None, seed=0, dp=None):
            seen.update(cfg=cfg, dtype=dtype)

    import tensorflowasr_amd.rnnt as rnnt_mod

    monkeypatch.setattr(rnnt_mod, "RnnTransducer", Fake)
    m = base_model.model_from_config(fixture)
    assert isinstance(m, Fake) and seen["cfg"] == configs.rnnt(vocab_size=1000) and seen["dtype"] == torch.bfloat16
    from tensorflowasr_amd.conformer import ConformerEncoderMixin
    from tensorflowasr_amd.transducer import TransducerModel

    assert issubclass(rnnt_mod.RnnEncoderMixin, object) and rnnt_mod.RnnTransducer is Fake
    monkeypatch.undo()
    assert issubclass(rnnt_mod.RnnTransducer, TransducerModel) and not issubclass(rnnt_mod.RnnTransducer, ConformerEncoderMixin)
    assert issubclass(rnnt_mod.RnnTransducer, rnnt_mod.RnnEncoderMixin)
    for name in ("train_step", "loss_and_backward", "compile"):
        assert getattr(rnnt_mod.RnnTransducer, name) is rnnt_mod.RnnEncoderMixin._inference_only
    with pytest.raises(NotImplementedError):
        base_model.model_from_config({"class_name": "tensorflow_asr.models.transducer.rnnt>Other", "config": {}})


def test_checkpoint_paths_are_the_references_layer_names():
    cfg = C.tiny_config("ln")
    W = ParamStore(cfg, torch.device("cpu"), torch.float32, 1).export_keras()
    paths = checkpoint.to_keras(W, path_fn=checkpoint.rnnt_keras_path)
    for must in ("encoder/block_0/lstm/kernel", "encoder/block_2/lstm/recurrent_kernel", "encoder/block_1/lstm/bias", "encoder/block_1/ln/gamma",
                 "encoder/block_1/ln/beta", "encoder/block_2/projection/kernel", "encoder/block_0/projection/bias", "joint/enc/kernel",
                 "prediction/lstm_0/lstm_cell/kernel"):
        assert must in paths, must
    assert paths["encoder/block_1/lstm/kernel"].shape == (48, 128) and paths["encoder/block_2/lstm/kernel"].shape == (32, 128)
    assert paths["encoder/block_0/projection/kernel"].shape == (32, 16) and paths["joint/enc/kernel"].shape == (16, 40)
    assert not any("/ln/" in p for p in checkpoint.to_keras(ParamStore(C.tiny_config("noln"), torch.device("cpu"), torch.float32, 1).export_keras(),
                                                            path_fn=checkpoint.rnnt_keras_path) if p.startswith("encoder/"))
    back = checkpoint.from_keras(paths, W, path_fn=checkpoint.rnnt_keras_path)
    assert sorted(back) == sorted(W) and all(torch.equal(torch.as_tensor(back[k]), W[k]) for k in W)
    with pytest.raises(KeyError):
        checkpoint.rnnt_keras_path("enc/block_0/lstm/zz")
