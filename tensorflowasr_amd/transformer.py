"""Transformer CTC and transducer models on the HIP kernels and C ABI of the other models, inference only, offline and streamed.

Mirrors  tensorflow_asr.models.ctc.transformer.Transformer          (models/ctc/transformer.py:56-121: TransformerEncoder + TransformerDecoder)
         tensorflow_asr.models.transducer.transformer.Transformer   (models/transducer/transformer.py:21-120: the same encoder under Transducer)
         TransformerEncoder.call                                     (models/encoders/transformer.py:316-345)
         TransformerBlock.call                                       (:153-188)   norm_position post (shipped) and pre
         PointwiseFFN.call                                           (:54-57)     Dense(dff, relu) -> Dense(dmodel)
         Conv2dSubsampling.call / compute_mask                       (models/layers/subsampling.py:218-247)
         SinusoidalPositionalEncoding.call                           (models/layers/positional_encoding.py:69-85, table :31-52)
         MultiHeadAttention.call, the mask and the masked softmax    (models/layers/multihead_attention.py:146-213, 331-423; general.py:25-41)
         Residual.call                                               (models/layers/residual.py:58-62)   x + factor * y

    features [B, T, F, 1] -> 2 x (Conv2D 3x3 stride 2 causal -> [BatchNorm] -> ReLU) -> merge_two_last_dims -> Dense(dmodel)
    -> + masked sinusoid table -> blocks
    block (post):  a = x + f * LN1(MHA(x));  y = a + f * LN2(FFN(a))          block (pre):  a = x + f * MHA(LN1(x));  y = a + f * FFN(LN2(a))

Per block: one GEMM for q|k|v (the Keras kernels [d, H, dh] are stored fused as [d, 3 H dh]), tfasr_attn_plain_fwd (csrc/attn_plain.hip:
nothing of size T x T in HBM; the f32 twin takes the unfused route instead, which measured faster: attention_route below), the output GEMM, tfasr_layernorm_fwd, the residual, Dense + ReLU as tfasr_conv1d_fwd with one tap, the
second Dense, LayerNorm, residual.  Post-norm with a residual factor other than 1 folds the factor into the LayerNorm's gamma / beta; pre-norm
takes the residual in the GEMM epilogue (res + beta * v).  The subsampling runs on the Conformer's pieces (tfasr_conv1_fwd, im2col + GEMM);
the inference BatchNorm (moving statistics, keras epsilon 1e-3) is folded once per weight load, in f32, to scale / shift and applied with
the ReLU by tfasr_channel_affine_fwd.  bf16 models read packed bf16 copies of the FFN's first kernel made at the same time; the cache is
dropped whenever the parameter store's weights change.

Masking is the reference's: only the QUERY rows carry the length mask.  A padded row attends uniformly over all T' keys, and because keys
are never masked its keys and values feed the valid rows of the next block - so a batch row is NOT the utterance run alone.  That is the
reference's behaviour on a padded batch and is reproduced, not masked away.  Which blocks see a length mask at all is the reference's
too: the attention layer reads the mask from its query tensor and then deletes it from that tensor (multihead_attention.py:368-373).
With norm_position "post" (the shipped setting) the query IS the block's input, from which the first Residual would afterwards inherit
its mask - so only block 0 sees the length mask, and from block 1 on every row attends under the causal / streaming mask alone; with "pre"
the query is the LayerNorm's output and every block sees it.  The reference's own classes, run over the keras shim, pin this
(tests/test_transformer_oracle.py, tests/golden/transformer_wiring.npz).  The chunked configuration (base-streaming.yml.j2) runs offline
with its mask; use_attention_auto_mask=False removes every mask, as in the reference (multihead_attention.py:375-384).

Decoders, forced alignment, evaluate, the precision switch (f32 twin by default, bf16 opt-in) and the .npz checkpoints are inherited.
A chunked config (use_attention_auto_mask, chunk_size, history_size >= 0) also streams: stream / stream_state / encode_chunk open the
sessions of tensorflowasr_amd/streaming.py (TransformerStreamState, transformer_encode_chunk: tfasr_stream_add_pe for the position rows
at each stream's offset, tfasr_stream_attn_plain_fwd for the chunk against the carried K / V rings).  Stream b holds the frames of that
utterance run ALONE: in a padded batch the padded frames of a shorter row's last chunk are visible keys (see Masking above).
Training, relmha, the Memory cache, unlimited history, look-ahead and .weights.h5 import are not built: train_step / loss_and_backward /
compile raise, and so do the three streaming entry points for a config that cannot be streamed.
"""
import numpy as np
import torch

from . import kernels as K
from .ctc_model import CtcModel
from .inference_only import InferenceOnlyEncoder
from .params import transformer_modules
from .transducer import TransducerModel


def sinusoid_table(T, d, interleave):
    """compute_sinusoid_position_encoding (positional_encoding.py:31-52) for positions 0 .. T-1, float32 arithmetic: [T, d]."""
    pos = np.arange(T, dtype=np.float32)
    mf = np.float32(1.0 / 10000.0)
    if interleave:
        ts = np.power(mf, (2 * (np.arange(d, dtype=np.float32) // 2)) / np.float32(d)).astype(np.float32)
        ang = pos[:, None] * ts[None, :]
        return np.where((np.arange(d) % 2 == 1)[None, :], np.cos(ang), np.sin(ang)).astype(np.float32)
    ts = np.power(mf, np.arange(0, d, 2, dtype=np.float32) / np.float32(d)).astype(np.float32)
    ang = pos[:, None] * ts[None, :]
    return np.concatenate([np.sin(ang), np.cos(ang)], -1).astype(np.float32)


class TransformerEncoderMixin(InferenceOnlyEncoder):
    """encoder_fwd and what it needs; mixed in front of CtcModel / TransducerModel"""

    encoder_kind = "transformer"
    _not_built = "the plain-attention backward and BatchNorm in batch-statistics mode are not built"

    # "fused": tfasr_attn_plain_fwd; "unfused": batched GEMMs + the softmax kernel with a zero position tensor (unfused_attention below);
    # "auto": the faster of the two as measured (profiles/transformer_timing.json, base config at T' = 250 and 875): in bf16 the fused
    # MFMA kernel (3.1x / 4.7x faster per layer); in f32 the fused kernel is a plain FMA kernel and runs at half the speed of the f32-MFMA
    # GEMMs around the softmax (0.34 against 0.14 ms, 2.87 against 1.40 ms per layer), so the f32 twin takes the unfused route - except
    # under the causal mask, which only the fused kernel has
    attention_route = "auto"

    def _init_encoder(self):
        super()._init_encoder()
        self.modules = transformer_modules(self.cfg)

    # ------------------------------------------------------------------------------------------- streaming (tensorflowasr_amd/streaming.py)
    # A config that cannot be streamed (full context, no auto mask, unlimited history, sizes beyond the kernel) is refused by
    # streaming.check_streamable before any argument is looked at: NotImplementedError, "... inference only ..." and the reason.
    def stream(self, batch_size=1, precision=None, max_tokens_per_frame=3, beam_width=0, max_frames=3000):
        """Incremental recognition session (streaming.StreamingRecognizer) of a chunked config (base-streaming.yml.j2): a step is
        4 * chunk_size feature frames; stream b gives the frames and tokens of that utterance run ALONE, however the samples arrive.
        Sessions, beams and their memory as ConformerTransducer.stream / ConformerCTC.stream."""
        from . import streaming

        streaming.check_streamable(self)
        return streaming.StreamingRecognizer(self, batch_size, precision, max_tokens_per_frame, beam_width, max_frames)

    # ------------------------------------------------------------------------------------------- constants derived from the weights
    def _ffn1_consts(self, p):
        d, ps, c = self._cache(), self.ps, self.cfg
        got = d.get((p, "ffn_1", self.dtype))
        if got is None:
            w = ps.p(p + "/pwffn/ffn_1/w").view(1, c.dmodel, c.dff)
            if self.dtype != torch.float32:
                w = K.conv1d_pack_weight(w)
            got = d[(p, "ffn_1", self.dtype)] = (w, ps.p(p + "/pwffn/ffn_1/b"))
        return got

    def _ln_consts(self, name):
        """(gamma, beta) of a post-norm LayerNorm with the residual factor folded in: x + f LN(y) = x + LN_{f gamma, f beta}(y)"""
        ps, f = self.ps, float(self.cfg.residual_factor)
        if f == 1.0 or self.cfg.norm_position != "post":
            return ps.p(name + "/g"), ps.p(name + "/b")
        d = self._cache()
        got = d.get((name, "scaled"))
        if got is None:
            got = d[(name, "scaled")] = ((ps.p(name + "/g") * f).contiguous(), (ps.p(name + "/b") * f).contiguous())
        return got

    def _pe(self, T):
        key = ("abs_pe", T)
        if key not in self._consts:
            self._consts[key] = torch.from_numpy(sinusoid_table(T, self.cfg.dmodel, bool(self.cfg.interleave_relpe))).to(self.device).contiguous()
        return self._consts[key]

    # ------------------------------------------------------------------------------------------- encoder
    def subsampling_fwd(self, feats):
        """Conv2dSubsampling.call + the encoder's `linear` (subsampling.py:218-230, encoders/transformer.py:324-325): [B, T0, F] -> [B*T2, d]"""
        ps = self.ps
        c0, c1 = self.modules["convs"]
        B = feats.shape[0]
        x = K.conv1_fwd(feats.contiguous(), ps.p(c0["name"] + "/w"), ps.p(c0["name"] + "/b"))  # [B, T1, F1, C0]
        x = K.channel_affine_fwd(x, *self._affine(c0["bn"]), relu=True, y=x)
        col = K.im2col_3x3s2(x)  # [B*T2*F2, 9 C0]
        T2, F2 = (x.shape[1] + 1) // 2, (x.shape[2] + 1) // 2
        y = K.matmul(col, ps.w2d(c1["name"] + "/w"), bias=ps.p(c1["name"] + "/b"))  # [B*T2*F2, C1]
        y = K.channel_affine_fwd(y, *self._affine(c1["bn"]), relu=True, y=y)
        merged = y.view(B * T2, F2 * c1["cout"])  # math_util.merge_two_last_dims
        return K.matmul(merged, ps.w2d("enc/linear/w"), bias=ps.p("enc/linear/b")), T2

    def _mask_args(self, index=0):
        c = self.cfg
        if not c.use_attention_auto_mask:  # no mask of any kind is computed (multihead_attention.py:375-384)
            return dict(use_mask=False, causal=False, chunk_size=None, history_size=None)
        # the query (length) mask reaches block 0 only under norm_position "post": see the module docstring
        return dict(use_mask=index == 0 or c.norm_position == "pre", causal=bool(c.use_attention_causal_mask), chunk_size=c.chunk_size,
                    history_size=c.history_size)

    def attention_fwd(self, qkv, B, T, lens_dev, index=0):
        """qkv [B*T, 3 H dh] -> context [B*T, H dh]; index = the block's position in the encoder"""
        c = self.cfg
        H, dh = int(c.num_heads), int(c.head_size)
        scale = 1.0 / float(np.sqrt(dh))
        m = self._mask_args(index)
        route = self.attention_route
        if route == "auto":
            route = "fused" if (self.dtype != torch.float32 or m["causal"]) else "unfused"
        if route == "fused":
            return K.attn_plain_fwd(qkv, lens_dev, B, H, T, dh, scale, **m)
        if m["causal"]:
            raise NotImplementedError("the unfused attention route has no causal mask")
        return unfused_attention(qkv, lens_dev, B, H, T, dh, scale, m["use_mask"], m["chunk_size"], m["history_size"])

    def block_fwd(self, x, p, B, T, lens_dev, index=0, attend=None):
        """one TransformerBlock: x [B*T, d] -> [B*T, d]; index = its position in the encoder (which decides whether it sees the length mask);
        attend(qkv) -> context stands in for attention_fwd (the streaming step: the chunk against the rings, T = chunk_size)"""
        ps, c = self.ps, self.cfg
        f, pre = float(c.residual_factor), c.norm_position == "pre"
        h = K.layernorm_fwd(x, ps.p(p + "/ln_1/g"), ps.p(p + "/ln_1/b"), save_stats=False)[0] if pre else x
        qkv = K.matmul(h, ps.w2d(p + "/mhsa/qkv/w"), bias=ps.p(p + "/mhsa/qkv/b"))
        ctxv = attend(qkv) if attend is not None else self.attention_fwd(qkv, B, T, lens_dev, index)
        if pre:
            a = K.matmul(ctxv, ps.w2d(p + "/mhsa/o/w"), bias=ps.p(p + "/mhsa/o/b"), res=x, beta=f)
            h = K.layernorm_fwd(a, ps.p(p + "/ln_2/g"), ps.p(p + "/ln_2/b"), save_stats=False)[0]
        else:
            o = K.matmul(ctxv, ps.w2d(p + "/mhsa/o/w"), bias=ps.p(p + "/mhsa/o/b"))
            a = K.add_act_fwd(x, K.layernorm_fwd(o, *self._ln_consts(p + "/ln_1"), save_stats=False)[0])
            h = a
        w1, b1 = self._ffn1_consts(p)
        z = K.conv1d_fwd(h.view(B, T, c.dmodel), w1, (1, c.dmodel, c.dff), bias=b1, relu=True).view(B * T, c.dff)
        if pre:
            return K.matmul(z, ps.w2d(p + "/pwffn/ffn_2/w"), bias=ps.p(p + "/pwffn/ffn_2/b"), res=a, beta=f)
        o = K.matmul(z, ps.w2d(p + "/pwffn/ffn_2/w"), bias=ps.p(p + "/pwffn/ffn_2/b"))
        return K.add_act_fwd(a, K.layernorm_fwd(o, *self._ln_consts(p + "/ln_2"), save_stats=False)[0])

    def embed_fwd(self, feats, flen):
        """subsampling, linear and the masked position table: -> x [B*T', d], T', lengths, lengths on the device"""
        x, T = self.subsampling_fwd(feats)
        B = feats.shape[0]
        lens = [self.cfg.encoder_length(n) for n in flen]
        lens_dev = self._h2d(lens)
        x = K.add_pe(x.view(B, T, self.cfg.dmodel), self._pe(T), lens_dev).view(B * T, self.cfg.dmodel)
        return x, T, lens, lens_dev

    def encoder_fwd(self, feats, flen, training, ctx):
        """TransformerEncoder.call (encoders/transformer.py:316-345): features [B, T0, F] -> [B*T', dmodel], T', lengths."""
        if training or ctx is not None:
            self._inference_only()
        x, T, lens, lens_dev = self.embed_fwd(feats, flen)
        B = feats.shape[0]
        for i, p in enumerate(self.modules["blocks"]):
            x = self.block_fwd(x, p, B, T, lens_dev, i)
        return x, T, lens, lens_dev


def unfused_attention(qkv, lens_dev, B, H, T, dh, scale, use_mask=True, chunk_size=None, history_size=None):
    """The same attention on the kernels the library had before csrc/attn_plain.hip: batched tfasr_gemm for scale * Q K^T, the
    relative-position softmax kernel fed a ZERO position tensor [B, H, T, 2T] (its read is part of this route's cost), batched
    tfasr_gemm for P V.  Scores and probabilities [B, H, T, T] go through HBM."""
    HD = H * dh
    ld = 3 * HD
    Tp = -(-T // 8) * 8
    content = torch.empty(B, H, T, Tp, dtype=qkv.dtype, device=qkv.device)
    q, k, v = qkv, qkv[:, HD:], qkv[:, 2 * HD:]
    K.gemm(q, k, content, T, T, dh, ld, ld, Tp, trans_b=True, alpha=scale, nb1=B, nb2=H, sA=(T * ld, dh), sB=(T * ld, dh), sD=(H * T * Tp, T * Tp))
    pos = torch.zeros(B, H, T, -(-2 * T // 8) * 8, dtype=qkv.dtype, device=qkv.device)
    probs = K.relattn_softmax_fwd(content, pos, lens_dev, T, use_mask=use_mask, probs=content, chunk_size=chunk_size, history_size=history_size)
    out = torch.empty(B * T, HD, dtype=qkv.dtype, device=qkv.device)
    K.gemm(probs, v, out, T, dh, T, Tp, ld, HD, nb1=B, nb2=H, sA=(H * T * Tp, T * Tp), sB=(T * ld, dh), sD=(T * HD, dh))
    return out


class TransformerCTC(TransformerEncoderMixin, CtcModel):
    _config_error = "TransformerCTC needs a TransformerConfig with head='ctc' (configs.transformer() / transformer_from_reference)"


class TransformerTransducer(TransformerEncoderMixin, TransducerModel):
    _config_error = "TransformerTransducer needs a TransformerConfig with head='transducer' (configs.transformer(head='rnnt'))"
