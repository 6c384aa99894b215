"""The tiny RNN-Transducer cases shared by tests/test_rnnt_encoder_oracle.py (CPU), the GPU tests and tools/gen_rnnt_fixtures.py: configs, seeded
weights, audio, the float64 oracle's results, and the run of the reference's OWN RnnTransducerEncoder over
oracle/keras_shim.reference_runtime() that tests/golden/rnnt_wiring.npz records.  Everything here runs without a GPU: the weights come
from a ParamStore on the CPU.

Settings (F = 16 mel bins, rnn_units 32, dmodel 16, V = 29):
    "ln"     three blocks, reductions [post, post, pre] by [3, 0, 2], LayerNorm in every block
    "noln"   two blocks, reductions [pre, pre] by [2, 0], no LayerNorm (the class default)
One batch of three utterances of 0.31 s, 0.5 s and 0.8 s: 31 / 50 / 80 feature frames (none a multiple of 6) -> 6 / 9 / 14 encoder frames
in "ln", 16 / 25 / 40 in "noln".  The reference's call_next is recorded for "ln" over the halves [0, 30) and [30, 80)."""
import importlib
import os

import numpy as np
import torch

from tensorflowasr_amd import checkpoint, configs
from tensorflowasr_amd.params import ParamStore

import rnnt_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIRING = os.path.join(ROOT, "tests", "golden", "rnnt_wiring.npz")
CONFIG_FIXTURE = os.path.join(ROOT, "tests", "golden", "rnnt_config.json")
SAMPLES = [4960, 8000, 12800]
FLEN = [31, 50, 80]
ELEN = {"ln": [6, 9, 14], "noln": [16, 25, 40]}
SPLIT = 30  # call_next's halves
SEED = 7
SETTINGS = {"ln": dict(reduction_positions=["post", "post", "pre"], reduction_factors=[3, 0, 2], nlayers=3, layer_norm=True),
            "noln": dict(reduction_positions=["pre", "pre"], reduction_factors=[2, 0], nlayers=2, layer_norm=False)}


def tiny_config(setting="ln", **over):
    kw = dict(SETTINGS[setting])
    kw.update(over)
    return configs.rnnt_tiny(**kw)


def make_weights(cfg, seed=SEED):
    """the initialiser's kernels, seeded non-trivial biases and LayerNorm parameters, a joint network that speaks"""
    W = ParamStore(cfg, torch.device("cpu"), torch.float32, seed).export_keras()
    g = torch.Generator().manual_seed(100 + seed)
    for name, t in W.items():
        leaf = name.rsplit("/", 1)[1]
        norm = "/ln/" in name
        if norm and leaf == "g":
            W[name] = torch.rand(t.shape, generator=g) + 0.5
        elif norm and leaf == "b":
            W[name] = torch.randn(t.shape, generator=g) * 0.3
        elif leaf == "b" and "/lstm/" not in name:
            W[name] = torch.randn(t.shape, generator=g) * 0.1
        elif name.endswith(("lstm/k", "lstm/rk")) and name.startswith("enc/"):
            W[name] = t * 2.0  # gates that leave the linear range
        elif name == "joint/vocab/w":
            W[name] = t * 6.0
    W["joint/vocab/b"] = W["joint/vocab/b"].clone()
    W["joint/vocab/b"][0] = -0.5  # the blank does not win every frame
    W["joint/vocab/b"][1] = -100.0  # never ' ' (class 1): a transcript survives the tokenizer's white-space normalisation unchanged
    return W


def numpy_weights(W):
    return {k: v.double().numpy() for k, v in W.items()}


def audio():
    rng = np.random.default_rng(5)
    sig = np.zeros((3, max(SAMPLES)), np.float32)
    for b, n in enumerate(SAMPLES):
        sig[b, :n] = np.clip(rng.standard_normal(n) * 0.1, -1, 1)
    return sig


def features(sig, cfg):
    """log-mel features [3, 80, F] float32 (the padded frames of a shorter utterance are those of its zero samples)"""
    from oracle import conformer_ref as R

    sc = dict(sample_rate=cfg.sample_rate, frame_ms=cfg.frame_ms, stride_ms=cfg.stride_ms, nfft=cfg.nfft, preemphasis=cfg.preemphasis,
              num_feature_bins=cfg.num_feature_bins, epsilon=cfg.epsilon)
    return np.asarray(R.log_mel(sig, sc), np.float32)


def greedy(enc, elen, W, batch=True):
    """the reference's greedy searches on encoder frames, float64: recognize_batch over the batch, or recognize_single per utterance"""
    from oracle import conformer_ref as R

    W64 = {k: v.double() for k, v in W.items() if k.startswith(("pred/", "joint/"))}
    e = torch.from_numpy(np.asarray(enc, np.float64))
    if batch:
        toks = R.recognize_batch(e, elen, W64)[0]
        return [[int(v) for v in row if v != 0] for row in toks]
    return [[int(v) for v in R.recognize_single(e[b:b + 1, :n], [n], W64)[0][0] if v != 0] for b, n in enumerate(elen)]


_REFS = {}


def reference(setting, **over):
    """features; the batch's encoder output in f64, in f32 (the f32 device path's yardstick) and with bf16 rounding (the floor); each
    utterance alone in f64 with its final LSTM states, on its rows of the batch's features ("alone": the encoder's statement) and from its
    own audio ("solo": what `encode` of the utterance and a stream hold); the greedy tokens of the batch and of each utterance from its
    own audio.  Computed once."""
    key = (setting, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key in _REFS:
        return _REFS[key]
    cfg = tiny_config(setting, **over)
    W = make_weights(cfg)
    Wn = numpy_weights(W)
    feats = features(audio(), cfg)
    trace = {}
    enc, elen, states = RO.encoder(feats, FLEN, cfg, Wn, trace=trace)
    enc32, _, _ = RO.encoder(feats, FLEN, cfg, Wn, dtype=np.float32)
    floor, _, _ = RO.encoder(feats, FLEN, cfg, Wn, rnd=RO.bf16_round, wrnd=RO.bf16_round)
    alone = [RO.encoder(feats[b:b + 1, :n], [n], cfg, Wn) for b, n in enumerate(FLEN)]
    # ... and from its own audio: the pre-emphasis of the first sample behind an utterance's end reads its last sample in a padded batch row
    # and nothing alone, so the last two feature frames of a shorter utterance differ between the two (the reference's front end on a batch)
    sig = audio()
    solo_feats = [features(sig[b:b + 1, :n], cfg) for b, n in enumerate(SAMPLES)]
    solo = [RO.encoder(f, [f.shape[1]], cfg, Wn) for f in solo_feats]
    pad = lambda rows: np.stack([np.pad(r, ((0, enc.shape[1] - r.shape[0]), (0, 0))) for r in rows])
    out = dict(cfg=cfg, W=W, Wn=Wn, feats=feats, flen=list(FLEN), enc=enc, enc32=enc32, floor=floor, elen=elen, states=states, trace=trace,
               alone=[a[0][0] for a in alone], alone_states=[a[2][0] for a in alone], solo_feats=solo_feats, solo=[a[0][0] for a in solo],
               solo_states=[a[2][0] for a in solo], tokens=greedy(enc, elen, W),
               tokens_alone=greedy(pad([a[0][0] for a in solo]), elen, W, batch=False))
    _REFS[key] = out
    return out


# ------------------------------------------------------------------------------------------------------------ the reference's classes
def have_reference():
    from oracle import keras_shim as KS

    return os.path.isfile(os.path.join(KS.REFERENCE_ROOT, "tensorflow_asr", "models", "encoders", "rnnt.py"))


def _build(mod, cfg, tf, KS, feats, flen):
    enc = mod.RnnTransducerEncoder(reduction_positions=list(cfg.reduction_positions), reduction_factors=list(cfg.reduction_factors),
                                   dmodel=cfg.encoder_dmodel, nlayers=cfg.nlayers, rnn_type=cfg.encoder_rnn_type, rnn_units=cfg.encoder_rnn_units,
                                   layer_norm=cfg.layer_norm, name="encoder")
    return enc, _inputs(tf, KS, feats, flen)


def _inputs(tf, KS, feats, flen):
    """features [B, T, F, 1] carrying the mask FeatureExtraction.compute_mask attaches in the model (feature_extraction.py:315-322):
    sequence_mask(frames of the utterance, frames of the batch).  The encoder's Reshape and every layer behind it pass a mask on; the LSTM of
    a block that has no `pre` reduction of its own reads it."""
    x = tf.convert_to_tensor(np.asarray(feats, np.float32)[..., None])
    KS.set_keras_mask(x, tf.sequence_mask(np.asarray(flen, np.int32), maxlen=x.shape[1], dtype=tf.bool))
    return x, tf.convert_to_tensor(np.asarray(flen, np.int32))


def reference_run(cfg, W, feats, flen, split=None):
    """The reference's own RnnTransducerEncoder with W assigned under the reference's layer names, run on the batch -> dict(encoder,
    lengths, arrays {Keras path: array}); with `split` also call_next over feats[:, :split] and feats[:, split:] from the zero state
    (next1 / len1 / states1, next2 / len2 / states2)."""
    from oracle import keras_shim as KS

    arrays = checkpoint.to_keras({k: v for k, v in W.items() if k.startswith("enc/")}, path_fn=checkpoint.rnnt_keras_path)
    flen = [int(n) for n in flen]
    with KS.reference_runtime() as (tf, keras):
        mod = importlib.import_module("tensorflow_asr.models.encoders.rnnt")
        enc, inputs = _build(mod, cfg, tf, KS, feats, flen)
        enc(inputs, training=False)  # builds every variable
        named = dict(enc.named_weights())
        assert sorted(named) == sorted(arrays), sorted(set(named) ^ set(arrays))  # the parameter set under the reference's own layer names
        for path, var in named.items():
            assert tuple(var.shape) == arrays[path].shape, path
            var.assign(arrays[path])
        out, out_len = enc(inputs, training=False)
        assert enc.time_reduction_factor == cfg.time_reduction_factor
        res = dict(encoder=np.asarray(out, np.float32), lengths=np.asarray(out_len, np.int32), arrays=arrays)
        for blk in enc.blocks:  # every LSTM of the run above saw a mask: the feature mask reached block 0
            assert blk.rnn.masks_seen[-1] is not None, blk.name
        if split is not None:
            st = enc.get_initial_state(len(flen))
            for tag, lo, hi in (("1", 0, split), ("2", split, np.asarray(feats).shape[1])):
                n = [min(max(v - lo, 0), hi - lo) for v in flen]
                x, xl = _inputs(tf, KS, np.asarray(feats)[:, lo:hi], n)
                o, ol, st = enc.call_next(x, xl, st)
                res["next" + tag], res["len" + tag], res["states" + tag] = np.asarray(o, np.float32), np.asarray(ol, np.int32), np.asarray(st, np.float32)
        return res
