"""Torch-CPU float64 restatement of the reference's DeepSpeech2 encoder, independent of the HIP path.

Follows  models/layers/feature_extraction.py:233-235   spectrogram: ln(|STFT|^2 + eps)[:, :, :num_feature_bins]
         keras Conv2D padding="same"                    out = ceil(L / s), total = max((out - 1) s + k - L, 0), left = total // 2 (what
                                                        oracle/keras_shim.py:_conv_nd restates)
         models/layers/convolution.py:132-144           Conv2D(padding="causal"): k - 1 zeros in front of BOTH axes, then a valid conv
         models/encoders/deepspeech2.py:105-117         ConvBlock.call: conv -> bn -> relu, length = conv_output_length over the time stride
         models/encoders/deepspeech2.py:119-133         ConvBlock.compute_mask: sequence_mask(reduced length, maxlen = reduced T)
         utils/math_util.py:282-305                     conv_output_length: ceil(n / stride) for "same" and "causal"
         models/encoders/deepspeech2.py:185-190         ConvModule.call: ... -> Reshape (merge_two_last_dims: [B, T, F * C], column f * C + c)
         models/encoders/deepspeech2.py:213-229,250-256 RnnBlock: LSTM(return_sequences, zero_output_for_mask=True) [in Bidirectional] [-> RowConv1D]
         keras LSTM                                     gates i, f, c, o; z = x W + h R + b; c = f c + i tanh(z_c); h = o tanh(c); a masked
                                                        step carries h and c and (zero_output_for_mask) emits zeros
         keras Bidirectional (merge "concat")           the backward layer walks the time-reversed sequence with the reversed mask, its
                                                        output is reversed back and concatenated behind the forward layer's
         models/encoders/deepspeech2.py:36-60           RowConv1D: DepthwiseConv1D(2 fw + 1, padding="causal", use_bias=False) -> bn -> relu
         models/encoders/deepspeech2.py:367-372         FcBlock: Dense -> relu
         models/ctc/deepspeech2.py:41-44                DeepSpeech2Decoder: Dense(vocab) "logits"
keras.layers.BatchNormalization at inference: (x - moving_mean) / sqrt(moving_variance + 1e-3) * gamma + beta.

W maps this package's parameter names (ParamStore.export_keras) to tensors.  The topology (layer names, which layers exist) is restated
here from the config, following the reference's constructors, and does not come from the package's own table
(params.deepspeech2_modules).  `rounder` (optional) is applied to every layer's output and `wround` to every kernel: with a bf16 round
trip they give the rounding floor of a bf16 pipeline."""
import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3


def pad_out(L, k, s, padding):
    """(left, right, out) of one axis"""
    out = -(-L // s)
    if padding == "same":
        tot = max((out - 1) * s + k - L, 0)
        return tot // 2, tot - tot // 2, out
    if padding == "causal":
        return k - 1, 0, out
    raise ValueError(padding)


def conv2d(x, w, strides, padding):
    """x [B, T, F, Cin], w [kh, kw, Cin, Cout] (Keras layout) -> [B, ceil(T / st), ceil(F / sf), Cout], float64."""
    x, w = torch.as_tensor(x).double(), torch.as_tensor(w).double()
    kh, kw = w.shape[:2]
    (tl, tr, To), (fl, fr, Fo) = pad_out(x.shape[1], kh, strides[0], padding), pad_out(x.shape[2], kw, strides[1], padding)
    xp = F.pad(x.permute(0, 3, 1, 2), (fl, fr, tl, tr))
    y = F.conv2d(xp, w.permute(3, 2, 0, 1).contiguous(), stride=tuple(strides)).permute(0, 2, 3, 1).contiguous()
    assert y.shape[1] == To and y.shape[2] == Fo
    return y


def affine(x, bias=None, scale=None, shift=None, relu=False):
    """the kernels' epilogue v = (x + bias) * scale + shift [relu], float64"""
    v = x.double()
    if bias is not None:
        v = v + bias.double()
    if scale is not None:
        v = v * scale.double()
    if shift is not None:
        v = v + shift.double()
    return torch.relu(v) if relu else v


def batchnorm(x, W, bn):
    g, b, mm, mv = (W[bn + s].double() for s in ("/g", "/b", "/mm", "/mv"))
    return (x - mm) / torch.sqrt(mv + BN_EPS) * g + b


def reduced_length(n, cfg):
    for st, _ in cfg.conv_strides:
        n = (int(n) + st - 1) // st  # conv_output_length, padding in ("same", "causal")
    return n


def lstm(xg, rk, lengths, reverse=False, hround=None):
    """xg [B, T, 4P] = x W + b, rk [P, 4P] -> (y [B, T, P], h_last [B, P], c_last [B, P]); a step t >= lengths[b] carries the state and
    emits zeros; reverse walks t = T-1 .. 0 (the same as flipping sequence and mask, running forward, and flipping the output back).
    hround: rounding of the carried h (a bf16 pipeline hands a bf16 h to the next step)."""
    xg, rk = torch.as_tensor(xg).double(), torch.as_tensor(rk).double()
    B, T, P4 = xg.shape
    P = P4 // 4
    h, c = torch.zeros(B, P, dtype=torch.float64), torch.zeros(B, P, dtype=torch.float64)
    y = torch.zeros(B, T, P, dtype=torch.float64)
    lengths = torch.as_tensor(np.asarray(lengths)).long()
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        z = xg[:, t] + h @ rk
        i, f, g, o = torch.sigmoid(z[:, :P]), torch.sigmoid(z[:, P:2 * P]), torch.tanh(z[:, 2 * P:3 * P]), torch.sigmoid(z[:, 3 * P:])
        cn = f * c + i * g
        hn = o * torch.tanh(cn)
        m = (t < lengths)[:, None]
        y[:, t] = torch.where(m, hn, torch.zeros_like(hn))
        if hround is not None:
            hn = hround(hn)
        h, c = torch.where(m, hn, h), torch.where(m, cn, c)
    return y, h, c


def lstm_infer(xg, rk, lengths, ndir, hround=None):
    """the entry point's layout: xg [B, T, ndir * 4P], rk [ndir, P, 4P] -> y [B, T, ndir * P], h_last, c_last [ndir, B, P]"""
    xg, rk = torch.as_tensor(xg).double(), torch.as_tensor(rk).double()
    P = rk.shape[1]
    outs = [lstm(xg[:, :, d * 4 * P:(d + 1) * 4 * P], rk[d], lengths, reverse=d == 1, hround=hround) for d in range(ndir)]
    return torch.cat([o[0] for o in outs], -1), torch.stack([o[1] for o in outs]), torch.stack([o[2] for o in outs])


def rowconv(x, w):
    """causal depthwise conv: x [B, T, C], w [K, C] -> y[t] = sum_k w[k] x[t - (K - 1) + k]"""
    x, w = x.double(), w.double()
    K = w.shape[0]
    xp = F.pad(x.transpose(1, 2), (K - 1, 0))
    return F.conv1d(xp, w.t().reshape(-1, 1, K).contiguous(), groups=x.shape[2]).transpose(1, 2).contiguous()


def topology(cfg):
    """names in call order: DeepSpeech2Encoder.__init__ (:446-484) -> conv_module/block_i (ConvModule :166-181), rnn_module/block_i
    (RnnModule :292-308) with `blstm` = Bidirectional(LSTM named "lstm") whose sub-layers keras names forward_lstm / backward_lstm, or a
    plain `lstm`, and `rowconv` only when not bidirectional and rnn_rowconv > 0 (:231); fc_module/block_i (FcModule :394-406)."""
    convs = [dict(name=f"enc/conv_module/block_{i}", strides=cfg.conv_strides[i]) for i in range(len(cfg.conv_filters))]
    rnns = []
    for i in range(cfg.rnn_nlayers):
        p = f"enc/rnn_module/block_{i}/"
        rnns.append(dict(dirs=[p + "blstm/forward_lstm", p + "blstm/backward_lstm"] if cfg.rnn_bidirectional else [p + "lstm"],
                         rowconv=p + "rowconv" if (not cfg.rnn_bidirectional and cfg.rnn_rowconv > 0) else None))
    fcs = [f"enc/fc_module/block_{i}" for i in range(cfg.fc_nlayers)]
    return convs, rnns, fcs


def conv_block(x, name, strides, cfg, W, wround=None):
    wr = wround or (lambda t: t)
    y = conv2d(x, wr(W[name + "/conv2d/w"]), strides, cfg.conv_padding) + W[name + "/conv2d/b"].double()
    return torch.relu(batchnorm(y, W, name + "/bn"))


def rnn_block(x, r, lens, W, rounder=None, wround=None):
    rd, wr = rounder or (lambda t: t), wround or (lambda t: t)
    outs = []
    for d, name in enumerate(r["dirs"]):
        xg = rd(x.double() @ wr(W[name + "/k"]).double() + W[name + "/b"].double())
        outs.append(lstm(xg, wr(W[name + "/rk"]), lens, reverse=d == 1, hround=rounder)[0])
    y = rd(torch.cat(outs, -1))
    if r["rowconv"]:
        y = rd(rowconv(y, W[r["rowconv"] + "/conv/w"]))
        y = rd(torch.relu(batchnorm(y, W, r["rowconv"] + "/bn")))
    return y


def encoder(feats, flen, cfg, W, rounder=None, wround=None, trace=None):
    """feats [B, T, F], flen = feature frames per row -> (frames [B, T', dmodel] float64, reduced lengths).  trace (a dict) receives the
    input of every layer under its name, and the masks the LSTMs saw under "masks"."""
    rd, wr = rounder or (lambda t: t), wround or (lambda t: t)
    convs, rnns, fcs = topology(cfg)
    x = rd(torch.as_tensor(feats).double())[..., None]
    for m in convs:
        if trace is not None:
            trace[m["name"]] = x
        x = rd(conv_block(x, m["name"], m["strides"], cfg, W, wround))
    lens = [reduced_length(n, cfg) for n in flen]
    B, T = x.shape[:2]
    x = x.reshape(B, T, -1)
    mask = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    if trace is not None:
        trace["masks"] = []
    for i, r in enumerate(rnns):
        if trace is not None:
            trace[f"enc/rnn_module/block_{i}"] = x
            trace["masks"] += [mask] * len(r["dirs"])
        x = rnn_block(x, r, lens, W, rounder, wround)
    for name in fcs:
        if trace is not None:
            trace[name] = x
        x = rd(torch.relu(x @ wr(W[name + "/fc/w"]).double() + W[name + "/fc/b"].double()))
    return x, lens


def logits(enc, W):
    return enc.double() @ W["dec/logits/w"].double() + W["dec/logits/b"].double()


def spectrogram(signal, cfg):
    """FeatureExtraction.call with feature_type "spectrogram" (feature_extraction.py:170-175 pre-emphasis, :206-209 |STFT|^2 with a
    periodic Hann window and pad_end, :214-218 natural log of S + eps, :233-235 the first num_feature_bins bins): [B, N] -> [B, T0, F] f64"""
    from oracle import conformer_ref as R  # the f32 pre-emphasis / window / power of the log-mel oracle (R.log_mel), minus the mel matrix

    x = R.preemphasis(np.asarray(signal, np.float32), cfg.preemphasis)
    n, step = cfg.frame_length, cfg.frame_step
    B, N = x.shape
    T0 = -(-N // step)
    xp = np.pad(x, [[0, 0], [0, max(0, (T0 - 1) * step + n - N)]])
    idx = np.arange(T0)[:, None] * step + np.arange(n)[None, :]
    frames = xp[:, idx] * R.hann_periodic(n)[None, None, :]
    power = np.square(np.abs(np.fft.rfft(frames.astype(np.float64), n=cfg.nfft, axis=-1))).astype(np.float32)
    return torch.from_numpy(np.log(power + np.float32(cfg.epsilon)).astype(np.float64)[:, :, :cfg.num_feature_bins])


def bf16_round(t):
    return t.to(torch.bfloat16).double()
