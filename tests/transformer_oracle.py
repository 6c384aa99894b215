"""Torch-CPU float64 restatement of the reference's Transformer encoder (+ CTC decoder), independent of the HIP path.

Follows  models/layers/subsampling.py:163-247          Conv2dSubsampling: (Conv2D 3x3 stride 2 "causal" -> [BatchNormalization] -> relu) x 2,
                                                       merge_two_last_dims (column f * C + c), lengths = ceil(n / 2) per block; its
                                                       compute_mask = sequence_mask(reduced length): the mask every later layer sees
         models/layers/convolution.py:132-144          Conv2D(padding="causal"): k - 1 zeros in front of BOTH axes, then a valid conv
         models/encoders/transformer.py:316-345        TransformerEncoder.call: subsampling -> linear -> pe -> blocks
         models/layers/positional_encoding.py:31-52    compute_sinusoid_position_encoding, both `interleave` settings
         models/layers/positional_encoding.py:69-85    SinusoidalPositionalEncoding.call: outputs += pe * sequence_mask(length)
         models/encoders/transformer.py:153-188        TransformerBlock.call, norm_position "post" and "pre"; Residual: x + factor * y
         models/layers/multihead_attention.py:347-423  MultiHeadAttention.call: the key / value masks are stripped; query, key, value Dense
                                                       [d, H, dh]; keras _compute_attention: query * 1/sqrt(key_dim), scores, masked softmax,
                                                       scores @ value; attention_output Dense [H, dh, d]
         models/layers/multihead_attention.py:146-213, 331-345   mask = query_mask[:, :, None] & causal & streaming; which blocks HAVE
                                                       a query mask: query_masked() below
         models/layers/general.py:25-41                Softmax: masked scores are REPLACED by -1e9
         models/ctc/transformer.py:40-43               TransformerDecoder: Dense(vocab) "logits"
keras LayerNormalization / BatchNormalization epsilon 1e-3; BatchNorm at inference uses the moving statistics.

The attention here is stated through its consequences, not through the mask tensor: a valid query row takes the softmax over its
visible keys only (a replaced score is exp(-1e9 - max) = exactly 0 in f32 and f64, and the row always sees itself), a padded query row
(i >= length) has every score replaced and is uniform over ALL T keys whatever the causal / streaming mask says.  Keys are never masked
by length.  tests/test_transformer_oracle.py holds it against the literal [B, T, T] mask + masked_fill form and against the reference's
own classes.  lse = log sum exp over the visible keys; a padded row's constant score is dropped (log T), as the kernels do.

W maps this package's parameter names (ParamStore.export_keras: q / k / v kernels [d, H, dh], output kernel [H, dh, d]) to tensors.
The topology is restated from the config.  dtype = torch.float32 runs the same arithmetic in f32 (the yardstick of the f32 device path);
`rounder` is applied to every stored activation and to the probabilities before P V, `wround` to every kernel: with a bf16 round trip
they give the rounding floor of a bf16 pipeline."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-3


def _id(t):
    return t


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def sinusoid_pe(T, d, interleave, dtype=torch.float64):
    pos = torch.arange(T, dtype=dtype)
    if interleave:
        ts = torch.pow(torch.tensor(1.0 / 10000.0, dtype=dtype), (2 * torch.div(torch.arange(d, dtype=dtype), 2, rounding_mode="floor")) / d)
        ang = pos[:, None] * ts[None, :]
        odd = (torch.arange(d) % 2 == 1)[None, :]
        return torch.where(odd, torch.cos(ang), torch.sin(ang))
    ts = torch.pow(torch.tensor(1.0 / 10000.0, dtype=dtype), torch.arange(0, d, 2, dtype=dtype) / d)
    ang = pos[:, None] * ts[None, :]
    return torch.cat([torch.sin(ang), torch.cos(ang)], -1)


def add_pe(x, lens, interleave):
    B, T, d = x.shape
    pe = sinusoid_pe(T, d, interleave, x.dtype)
    m = (torch.arange(T)[None, :] < torch.as_tensor(np.asarray(lens)).long()[:, None]).to(x.dtype)
    return x + pe[None] * m[:, :, None]


def visible(i, T, causal=False, chunk=None, hist=None):
    """[lo, hi) of a VALID query row i: compute_streaming_mask's window ANDed with the lower triangle"""
    lo, hi = 0, T
    if chunk:
        c = (i // chunk) * chunk
        lo = 0 if (hist is None or hist < 0) else max(0, c - hist)
        hi = min(T, c + chunk)
    if causal:
        hi = min(hi, i + 1)
    return lo, hi


def attention(q, k, v, scale, lens=None, use_mask=True, causal=False, chunk=None, hist=None, pround=None, want_lse=False):
    """q, k, v [B, H, T, dh] -> context [B, H, T, dh] (and lse [B, H, T]), in the dtype of q"""
    B, H, T, dh = q.shape
    dt = q.dtype
    pr = pround or _id
    s = torch.matmul(q * scale, k.transpose(-1, -2))
    out = torch.zeros_like(q)
    lse = torch.zeros(B, H, T, dtype=dt)
    for b in range(B):
        n = T if (lens is None or not use_mask) else max(0, min(int(lens[b]), T))
        for i in range(T):
            if i >= n:
                p = torch.full((H, T), 1.0 / T, dtype=dt)
                out[b, :, i] = torch.matmul(pr(p)[:, None, :], v[b])[:, 0]
                lse[b, :, i] = math.log(T)
                continue
            lo, hi = visible(i, T, causal, chunk, hist)
            row = s[b, :, i, lo:hi]
            lse[b, :, i] = torch.logsumexp(row, -1)
            p = torch.softmax(row, -1)
            out[b, :, i] = torch.matmul(pr(p)[:, None, :], v[b, :, lo:hi])[:, 0]
    return (out, lse) if want_lse else out


def attention_qkv(qkv, B, H, T, dh, scale, **kw):
    """the kernel's layout: qkv [B*T, 3 H dh] (q|k|v column blocks) -> context [B*T, H dh]"""
    q, k, v = (qkv[:, j * H * dh:(j + 1) * H * dh].reshape(B, T, H, dh).permute(0, 2, 1, 3) for j in range(3))
    res = attention(q, k, v, scale, **kw)
    if isinstance(res, tuple):
        return res[0].permute(0, 2, 1, 3).reshape(B * T, H * dh), res[1]
    return res.permute(0, 2, 1, 3).reshape(B * T, H * dh)


def conv2d_causal_s2(x, w):
    """x [B, T, F, Cin], w [3, 3, Cin, Cout] -> [B, ceil(T / 2), ceil(F / 2), Cout]"""
    xp = F.pad(x.permute(0, 3, 1, 2), (2, 0, 2, 0))
    return F.conv2d(xp, w.permute(3, 2, 0, 1).contiguous(), stride=(2, 2)).permute(0, 2, 3, 1).contiguous()


def layer_norm(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + EPS) * g + b


def reduced_length(n):
    return -(-(-(-int(n) // 2)) // 2)


def query_masked(cfg, i):
    """Does block i's attention see the query (length) mask?  The layer takes it from the Keras mask of its query TENSOR and then deletes
    that mask from the tensor (multihead_attention.py:368-373).  Under norm_position "post" the query IS the block's input, the very
    tensor the first Residual reads its mask from afterwards (residual.py:58-62 via keras' compute_mask: the mask of the first input) - so
    block 0 is the only block that sees a length mask, and from block 1 on every row, padded ones included, attends under the causal /
    streaming mask alone.  Under "pre" the query is the LayerNorm's output, the block's input keeps its mask, and every block sees it.
    tests/test_transformer_oracle.py runs the reference's own classes against this."""
    return i == 0 or cfg.norm_position == "pre"


def mask_args(cfg, i=0):
    if not cfg.use_attention_auto_mask:
        return dict(use_mask=False, causal=False, chunk=None, hist=None)
    return dict(use_mask=query_masked(cfg, i), causal=bool(cfg.use_attention_causal_mask), chunk=cfg.chunk_size, hist=cfg.history_size)


def subsampling(feats, cfg, W, dtype=torch.float64, rounder=None, wround=None):
    rd, wr = rounder or _id, wround or _id
    g = lambda name: W[name].to(dtype)
    x = rd(torch.as_tensor(feats).to(dtype))[..., None]
    for i in range(2):
        p = f"enc/subsampling/block_{i}/"
        x = rd(conv2d_causal_s2(x, wr(g(p + f"conv_{i}/w"))) + g(p + f"conv_{i}/b"))
        if cfg.sub_norm == "batch":
            bn = p + f"bn_{i}"
            x = (x - g(bn + "/mm")) / torch.sqrt(g(bn + "/mv") + EPS) * g(bn + "/g") + g(bn + "/b")
        x = rd(torch.relu(x))
    B, T = x.shape[:2]
    x = x.reshape(B, T, -1)
    return rd(x @ wr(g("enc/linear/w")) + g("enc/linear/b"))


def mha(x, p, cfg, W, lens, dtype, rd, wr, index=0):
    B, T, d = x.shape
    H, dh = int(cfg.num_heads), int(cfg.head_size)
    g = lambda name: W[name].to(dtype)
    q, k, v = (rd(torch.einsum("btd,dhe->bhte", x, wr(g(f"{p}/mhsa/{n}/w"))) + g(f"{p}/mhsa/{n}/b")[None, :, None, :]) for n in "qkv")
    c = rd(attention(q, k, v, 1.0 / math.sqrt(dh), lens=lens, pround=None if rd is _id else rd, **mask_args(cfg, index)))
    return rd(torch.einsum("bhte,hed->btd", c, wr(g(p + "/mhsa/o/w"))) + g(p + "/mhsa/o/b"))


def block(x, p, cfg, W, lens, dtype=torch.float64, rounder=None, wround=None, index=0):
    """one TransformerBlock; index = its position in the encoder (query_masked)"""
    rd, wr = rounder or _id, wround or _id
    g = lambda name: W[name].to(dtype)
    f, pre = float(cfg.residual_factor), cfg.norm_position == "pre"
    ln1 = lambda t: rd(layer_norm(t, g(p + "/ln_1/g"), g(p + "/ln_1/b")))
    ln2 = lambda t: rd(layer_norm(t, g(p + "/ln_2/g"), g(p + "/ln_2/b")))
    y = mha(ln1(x) if pre else x, p, cfg, W, lens, dtype, rd, wr, index)
    a = rd(x + f * (y if pre else ln1(y)))
    h = ln2(a) if pre else a
    z = rd(torch.relu(h @ wr(g(p + "/pwffn/ffn_1/w")) + g(p + "/pwffn/ffn_1/b")))
    z = rd(z @ wr(g(p + "/pwffn/ffn_2/w")) + g(p + "/pwffn/ffn_2/b"))
    return rd(a + f * (z if pre else ln2(z)))


def embed(feats, flen, cfg, W, dtype=torch.float64, rounder=None, wround=None):
    """subsampling, linear, masked position table: -> x [B, T', d], reduced lengths"""
    rd = rounder or _id
    x = subsampling(feats, cfg, W, dtype, rounder, wround)
    lens = [reduced_length(n) for n in flen]
    return rd(add_pe(x, lens, bool(cfg.interleave_relpe))), lens


def encoder(feats, flen, cfg, W, dtype=torch.float64, rounder=None, wround=None, trace=None):
    """feats [B, T, F], flen = feature frames per row -> (frames [B, T', dmodel], reduced lengths); trace (a dict) receives the input of
    every block under its prefix"""
    x, lens = embed(feats, flen, cfg, W, dtype, rounder, wround)
    for i in range(int(cfg.num_blocks)):
        p = f"enc/block_{i}"
        if trace is not None:
            trace[p] = x
        x = block(x, p, cfg, W, lens, dtype, rounder, wround, index=i)
    return x, lens


def logits(enc, W, dtype=torch.float64):
    return enc.to(dtype) @ W["dec/logits/w"].to(dtype) + W["dec/logits/b"].to(dtype)
