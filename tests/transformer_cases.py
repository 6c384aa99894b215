"""The tiny Transformer cases shared by tests/test_transformer_oracle.py (CPU), tests/test_transformer_gpu.py and
tools/gen_transformer_fixtures.py: configs, seeded weights, audio, the float64 oracle's results, and the run of the reference's OWN
TransformerEncoder + TransformerDecoder over oracle/keras_shim.reference_runtime() that tests/golden/transformer_wiring.npz records.
Everything here runs without a GPU: the weights come from a ParamStore on the CPU."""
import importlib
import os

import numpy as np
import torch

from tensorflowasr_amd import checkpoint, configs
from tensorflowasr_amd.params import ParamStore

import transformer_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIRING = os.path.join(ROOT, "tests", "golden", "transformer_wiring.npz")
CONFIG_FIXTURE = os.path.join(ROOT, "tests", "golden", "transformer_config.json")
SAMPLES = [4960, 8000, 12800]  # 0.31 s, 0.5 s, 0.8 s -> 31 / 50 / 80 feature frames -> 8 / 13 / 20 encoder frames
ELEN = [8, 13, 20]
SEED = 7  # a seed whose oracle logits keep the top-two margin asserted in tests/test_transformer_oracle.py and say > 3 tokens per utterance
SETTINGS = {"full": {}, "chunked": dict(chunk_size=4, history_size=8)}  # the shipped window's proportions (history = 2 chunks) at T' = 20


def tiny_config(setting="full", head="ctc", **over):
    kw = dict(SETTINGS[setting])
    kw.update(over)
    return configs.transformer_tiny(head=head, **kw)


def make_weights(cfg, seed=SEED):
    """the initialiser's kernels, seeded non-trivial biases, LayerNorm / BatchNorm parameters and moving statistics; a decoder that never
    says ' ' (class 1), so a transcript survives the tokenizer's white-space normalisation unchanged"""
    W = ParamStore(cfg, torch.device("cpu"), torch.float32, seed).export_keras()
    g = torch.Generator().manual_seed(100 + seed)
    for name, t in W.items():
        leaf = name.rsplit("/", 1)[1]
        norm = "/bn_" in name or "/ln_" in name or name.startswith("pred/ln")
        if norm and leaf == "g" or leaf == "mv":
            W[name] = torch.rand(t.shape, generator=g) + 0.5
        elif norm and leaf == "b" or leaf == "mm":
            W[name] = torch.randn(t.shape, generator=g) * 0.3
        elif leaf == "b" and not name.startswith("pred/lstm"):
            W[name] = torch.randn(t.shape, generator=g) * 0.1
        elif name.endswith(("mhsa/q/w", "mhsa/k/w")):
            W[name] = t * 3.0  # scores of a few units: a softmax that is far from uniform
        elif name.endswith("logits/w"):
            W[name] = t * 3.0
    if "enc/subsampling/block_0/bn_0/mm" in W:
        W["enc/subsampling/block_0/bn_0/mm"] = W["enc/subsampling/block_0/bn_0/mm"] - 4.0  # log-mel features are O(ln power): centred
    if "dec/logits/b" in W:
        W["dec/logits/b"] = W["dec/logits/b"].clone()
        W["dec/logits/b"][1] = -100.0  # (far below every other logit, and small enough not to set the f32 error of the logits)
    return W


def audio():
    rng = np.random.default_rng(5)
    sig = np.zeros((3, max(SAMPLES)), np.float32)
    for b, n in enumerate(SAMPLES):
        sig[b, :n] = np.clip(rng.standard_normal(n) * 0.1, -1, 1)
    return sig


def features(sig, cfg):
    from oracle import conformer_ref as R

    sc = dict(sample_rate=cfg.sample_rate, frame_ms=cfg.frame_ms, stride_ms=cfg.stride_ms, nfft=cfg.nfft, preemphasis=cfg.preemphasis,
              num_feature_bins=cfg.num_feature_bins, epsilon=cfg.epsilon)
    return torch.from_numpy(R.log_mel(sig, sc).astype(np.float64))


def collapse(logits, n, blank=0):
    path = np.argmax(np.asarray(logits[:n]), -1)
    return [int(c) for k, c in enumerate(path) if c != blank and (k == 0 or c != path[k - 1])]


def _valid(t, elen):
    return np.concatenate([np.asarray(t[b, :n], np.float64).reshape(n, -1) for b, n in enumerate(elen)])


def reference(setting, sig=None, cfg=None, W=None, feats=None):
    """features, per-block inputs, encoder output and logits in f64; the same in f32 (the f32 device path's yardstick) and with bf16 rounding
    (the floor); the greedy tokens, the smallest top-two logit margin over the valid frames, and the f32 run's largest logit error"""
    cfg = cfg or tiny_config(setting)
    W = W or make_weights(cfg)
    feats = features(audio() if sig is None else sig, cfg) if feats is None else feats
    flen = [-(-n // cfg.frame_step) for n in SAMPLES]
    trace = {}
    enc, elen = TO.encoder(feats, flen, cfg, W, trace=trace)
    enc32, _ = TO.encoder(feats, flen, cfg, W, dtype=torch.float32)
    floor, _ = TO.encoder(feats, flen, cfg, W, rounder=TO.bf16_round, wround=TO.bf16_round)
    out = dict(cfg=cfg, W=W, feats=feats, flen=flen, enc=enc, enc32=enc32, floor=floor, elen=elen, trace=trace)
    if cfg.head == "ctc":
        lg, lg32 = TO.logits(enc, W), TO.logits(enc32, W, torch.float32)
        top2 = torch.topk(lg, 2, -1).values
        out.update(logits=lg, logits32=lg32, margin=min(float((top2[b, :n, 0] - top2[b, :n, 1]).min()) for b, n in enumerate(elen)),
                   logit_err32=float(np.abs(_valid(lg32, elen) - _valid(lg, elen)).max()),
                   tokens=[collapse(lg[b].numpy(), elen[b]) for b in range(len(elen))])
    return out


# ------------------------------------------------------------------------------------------------------------ the reference's classes
def have_reference():
    from oracle import keras_shim as KS

    return os.path.isdir(os.path.join(KS.REFERENCE_ROOT, "tensorflow_asr", "models", "encoders"))


def _shim_mha(KS):
    class MultiHeadAttention(KS.MultiHeadAttention):
        """The shim's MultiHeadAttention has the projections and the mask helpers but not keras' dot-product core, which only the plain
        attention calls.  As keras documents it: the query is scaled by 1 / sqrt(key_dim), scores = einsum(dot_product_equation, key,
        query), the masked softmax, (dropout: inference, none), output = einsum(combine_equation, scores, value)."""

        def _compute_attention(self, query, key, value, attention_mask=None, training=None, return_attention_scores=False):
            q = np.asarray(query, np.float64) * self._inverse_sqrt_key_dim
            scores = KS._t(np.einsum(self._dot_product_equation, np.asarray(key, np.float64), q).astype(np.float32))
            scores = self._masked_softmax(scores, attention_mask)
            out = np.einsum(self._combine_equation, np.asarray(scores, np.float64), np.asarray(value, np.float64)).astype(np.float32)
            return KS._t(out), scores

    return MultiHeadAttention


def reference_run(cfg, W, feats, flen):
    """The reference's own TransformerEncoder + TransformerDecoder with W assigned under the reference's layer names, run on the batch.
    -> (encoder output [B, T', d], reduced lengths, logits [B, T', V], {Keras path: array} as assigned)"""
    from oracle import keras_shim as KS

    arrays = checkpoint.to_keras({k: v for k, v in W.items() if k.startswith(("enc/", "dec/"))}, path_fn=checkpoint.transformer_keras_path)
    sub = dict(type="conv2d", filters=list(cfg.sub_filters), kernels=[3, 3], strides=[2, 2], paddings=["causal", "causal"],
               norms=[cfg.sub_norm] * 2, activations=["relu", "relu"])
    import types

    # models/ctc/transformer.py imports CtcModel (and with it the losses, which need libraries that are not here) only as the base of the
    # model class; the decoder layer this run needs stands alone
    base_ctc = types.ModuleType("tensorflow_asr.models.ctc.base_ctc")
    base_ctc.CtcModel = type("CtcModel", (), {})
    with KS.reference_runtime(stubs={"tensorflow_asr.models.ctc.base_ctc": base_ctc}) as (tf, keras):
        keras.layers.MultiHeadAttention = _shim_mha(KS)
        enc_mod = importlib.import_module("tensorflow_asr.models.encoders.transformer")
        ctc_mod = importlib.import_module("tensorflow_asr.models.ctc.transformer")
        enc = enc_mod.TransformerEncoder(subsampling=sub, num_blocks=cfg.num_blocks, dmodel=cfg.dmodel, dff=cfg.dff, num_heads=cfg.num_heads,
                                         head_size=cfg.head_size, dropout=0.0, mha_type=cfg.mha_type, norm_position=cfg.norm_position,
                                         residual_factor=cfg.residual_factor, interleave_relpe=cfg.interleave_relpe,
                                         use_attention_causal_mask=cfg.use_attention_causal_mask,
                                         use_attention_auto_mask=cfg.use_attention_auto_mask, pwffn_activation=cfg.pwffn_activation,
                                         history_size=cfg.history_size, chunk_size=cfg.chunk_size, name="encoder")
        dec = ctc_mod.TransformerDecoder(vocab_size=cfg.vocab_size, name="decoder")
        inputs = (tf.convert_to_tensor(np.asarray(feats, np.float32)[..., None]), tf.convert_to_tensor(np.asarray(flen, np.int32)))
        dec(enc(inputs, training=False), training=False)  # builds every variable
        named = dict(enc.named_weights())
        named.update(dec.named_weights())
        assert sorted(named) == sorted(arrays), sorted(set(named) ^ set(arrays))  # the parameter set under the reference's own layer names
        for path, var in named.items():
            assert tuple(var.shape) == arrays[path].shape, path
            var.assign(arrays[path])
        out, out_len = enc(inputs, training=False)
        lg, _ = dec((out, out_len), training=False)
        assert enc.time_reduction_factor == cfg.time_reduction_factor
        return np.asarray(out, np.float32), np.asarray(out_len).tolist(), np.asarray(lg, np.float32), arrays
