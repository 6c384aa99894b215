"""The tiny DeepSpeech2 cases shared by tests/test_ds2_oracle.py (CPU) and tests/test_ds2_gpu.py: configs, seeded weights, audio, and the
float64 oracle's results.  Everything here runs without a GPU: the weights come from a ParamStore on the CPU."""
import numpy as np
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd.params import ParamStore

import ds2_oracle as DO

SAMPLES = [4960, 8000, 12800]  # 0.31 s, 0.5 s, 0.8 s
SEED = {"bi": 11, "uni": 12}  # seeds whose oracle logits have a top-two margin > 1e-3 on every valid frame and say > 3 tokens per utterance


def tiny_config(variant="bi", **over):
    kw = dict(vocab_size=29, num_feature_bins=16, feature_type="spectrogram", conv_kernels=[[5, 7], [3, 5]], conv_strides=[[2, 2], [1, 2]],
              conv_filters=[16, 16], rnn_nlayers=2, rnn_units=32, fc_nlayers=1, fc_units=64)
    if variant == "bi":
        kw.update(conv_padding="same", rnn_bidirectional=True, rnn_rowconv=0)
    else:
        kw.update(conv_padding="causal", rnn_bidirectional=False, rnn_rowconv=2)
    kw.update(over)
    return configs.deepspeech2_tiny(**kw)


def make_weights(cfg, seed=None):
    """the initialiser's kernels, seeded non-trivial biases and BatchNorm state; LSTM kernels scaled up so that the gates leave their
    linear range; a decoder that never says ' ' (class 1), so a transcript survives the tokenizer's white-space normalisation unchanged"""
    seed = SEED["bi" if cfg.rnn_bidirectional else "uni"] if seed is None else seed
    W = ParamStore(cfg, torch.device("cpu"), torch.float32, seed).export_keras()
    g = torch.Generator().manual_seed(100 + seed)
    for name, t in W.items():
        if name.endswith("bn/g"):
            W[name] = torch.rand(t.shape, generator=g) + 0.5
        elif name.endswith("bn/b") or name.endswith("bn/mm"):
            W[name] = torch.randn(t.shape, generator=g) * 0.3
        elif name.endswith("bn/mv"):
            W[name] = torch.rand(t.shape, generator=g) + 0.5
        elif name.endswith("conv2d/b") or name.endswith("fc/b"):
            W[name] = torch.randn(t.shape, generator=g) * 0.1
        elif name.endswith("lstm/b"):
            W[name] = t + torch.randn(t.shape, generator=g) * 0.2
        elif name.endswith("lstm/k") or name.endswith("logits/w"):
            W[name] = t * 3.0
        elif name.endswith("rowconv/conv/w"):
            W[name] = torch.randn(t.shape, generator=g) * 0.5
    # spectrogram features are O(ln power) ~ -14 .. 3: the first block's BatchNorm centres them
    W["enc/conv_module/block_0/bn/mm"] = W["enc/conv_module/block_0/bn/mm"] - 2.0
    W["dec/logits/b"] = W["dec/logits/b"].clone()
    W["dec/logits/b"][1] = -1e4
    return W


def audio():
    rng = np.random.default_rng(5)
    sig = np.zeros((3, max(SAMPLES)), np.float32)
    for b, n in enumerate(SAMPLES):
        sig[b, :n] = np.clip(rng.standard_normal(n) * 0.1, -1, 1)
    return sig


def collapse(logits, n, blank=0):
    path = np.argmax(np.asarray(logits[:n]), -1)
    return [int(c) for k, c in enumerate(path) if c != blank and (k == 0 or c != path[k - 1])]


def reference(variant, sig):
    """features, encoder output, logits, the per-layer inputs, the bf16 floor, the greedy tokens and the smallest top-two logit margin
    over the valid frames"""
    cfg = tiny_config(variant)
    W = make_weights(cfg)
    feats = DO.spectrogram(sig, cfg)
    flen = [-(-n // cfg.frame_step) for n in SAMPLES]
    trace = {}
    enc, elen = DO.encoder(feats, flen, cfg, W, trace=trace)
    floor, _ = DO.encoder(feats, flen, cfg, W, rounder=DO.bf16_round, wround=DO.bf16_round)
    lg = DO.logits(enc, W)
    top2 = torch.topk(lg, 2, -1).values
    margin = min(float((top2[b, :n, 0] - top2[b, :n, 1]).min()) for b, n in enumerate(elen))
    return dict(cfg=cfg, W=W, feats=feats, enc=enc, logits=lg, trace=trace, floor=floor, elen=elen, margin=margin,
                tokens=[collapse(lg[b].numpy(), elen[b]) for b in range(3)])
