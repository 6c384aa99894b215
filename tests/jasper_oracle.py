"""Torch-CPU float64 restatement of the reference's Jasper encoder, independent of the HIP path: torch.nn.functional.conv1d on
left-padded input.

Follows  models/layers/convolution.py:41-81        Conv1D(padding="causal"): dilation * (K - 1) zero rows in front, then a valid conv
         models/encoders/jasper.py:61-67           JasperSubBlock.call: conv1d -> bn -> relu (dropout is the identity at inference)
         models/encoders/jasper.py:102-105         JasperResidual.call: pointwise_conv1d -> bn
         models/encoders/jasper.py:152-161         JasperSubBlockResidual.call: conv1d -> bn -> add every residual branch -> relu
         models/encoders/jasper.py:210-220         JasperBlock.call: dense blocks append their input to the running residual list
         models/encoders/jasper.py:322-334         JasperEncoder.call
         models/ctc/jasper.py:45-48                JasperDecoder.call: Conv1D(vocab, 1) = a matrix product per frame
         models/layers/feature_extraction.py:214-218   log base 10 of the mel energies
keras.layers.BatchNormalization at inference: (x - moving_mean) / sqrt(moving_variance + 1e-3) * gamma + beta.

W maps this package's parameter names (ParamStore.export_keras) to tensors.  The topology (layer order, strides, which block inputs
feed which residual branch) is restated here from the config by `topology`, following the reference's constructors line by line, and
does not come from the package's own table (params.jasper_modules).  `rounder` (optional) is applied to every layer's output: with a bf16 round trip it gives the rounding floor of a
bf16 pipeline."""
import math

import torch
import torch.nn.functional as F

BN_EPS = 1e-3


def conv1d_causal(x, w, stride=1, dilation=1):
    """x [B, T, Cin], w [K, Cin, Cout] (Keras layout) -> [B, ceil(T / stride), Cout], float64."""
    x, w = x.double(), w.double()
    K = w.shape[0]
    xp = F.pad(x.transpose(1, 2), (dilation * (K - 1), 0))
    return F.conv1d(xp, w.permute(2, 1, 0).contiguous(), stride=stride, dilation=dilation).transpose(1, 2).contiguous()


def batchnorm(x, W, bn):
    g, b, mm, mv = (W[bn + s].double() for s in ("/g", "/b", "/mm", "/mv"))
    return (x - mm) / torch.sqrt(mv + BN_EPS) * g + b


def topology(cfg):
    """[dict(name, K, stride, dilation, residuals=[(name, source)])] in call order, `source` indexing the running residual list.
    JasperEncoder.__init__ (:264-317): first_block, block_{i} (nsubblocks - 1 plain sub-blocks "subordinate_j" and a last one with
    i + 1 residual branches when dense, else one: :183-206, :284), second_block, third_block.  JasperBlock.call (:210-220): a dense block
    appends ITS input to the shared list and hands the whole list on (branch r reads entry r); otherwise the branch reads the block's
    input only."""
    out = [dict(name="enc/first_block", K=cfg.first_additional_block_kernels, stride=cfg.first_additional_block_strides,
                dilation=cfg.first_additional_block_dilation, residuals=[], block_input=False)]
    for i, k in enumerate(cfg.block_kernels):
        for j in range(cfg.nsubblocks):
            last = j == cfg.nsubblocks - 1
            name = f"enc/block_{i}/subordinate_{j}"
            res = [(f"{name}/residual_{r}", r if cfg.dense else i) for r in range(i + 1 if cfg.dense else 1)] if last else []
            out.append(dict(name=name, K=k, stride=1, dilation=1, residuals=res, block_input=j == 0))
    for which in ("second", "third"):
        out.append(dict(name=f"enc/{which}_block", K=getattr(cfg, which + "_additional_block_kernels"),
                        stride=getattr(cfg, which + "_additional_block_strides"), dilation=getattr(cfg, which + "_additional_block_dilation"),
                        residuals=[], block_input=False))
    return out


def layer(x, m, residuals, W, wround=None):
    """one module of params.jasper_modules: conv -> bn [-> + residual branches] -> relu"""
    wr = wround or (lambda t: t)
    y = batchnorm(conv1d_causal(x, wr(W[m["name"] + "/conv1d/w"]), m["stride"], m["dilation"]) + W[m["name"] + "/conv1d/b"].double(), W,
                  m["name"] + "/bn")
    for rname, src in m["residuals"]:
        y = y + batchnorm(conv1d_causal(residuals[src], wr(W[rname + "/pointwise_conv1d/w"])) + W[rname + "/pointwise_conv1d/b"].double(), W,
                          rname + "/bn")
    return torch.relu(y)


def encoder(feats, cfg, W, rounder=None, wround=None, trace=None):
    """feats [B, T, F] -> [B, ceil(T / 2), dmodel] float64.  trace (a list) receives (x, residuals) at the input of every layer."""
    rd = rounder or (lambda t: t)
    x, residuals = rd(feats.double()), []
    for m in topology(cfg):
        if m["block_input"]:
            residuals.append(x)  # (not dense: entry i is block i's input, the only one its branch reads)
        if trace is not None:
            trace.append((x, list(residuals)))
        x = rd(layer(x, m, residuals, W, wround))
    return x


def logits(enc, W):
    return enc.double() @ W["dec/logits/w"].double() + W["dec/logits/b"].double()


def log10_features(natural_log_feats):
    return torch.as_tensor(natural_log_feats).double() / math.log(10.0)


def bf16_round(t):
    return t.to(torch.bfloat16).double()
