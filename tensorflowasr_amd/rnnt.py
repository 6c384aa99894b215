"""RNN-Transducer (LSTM encoder) on the HIP kernels and C ABI of the other models, inference only.

Mirrors  tensorflow_asr.models.transducer.rnnt.RnnTransducer   (models/transducer/rnnt.py:21-105: RnnTransducerEncoder under Transducer)
         RnnTransducerEncoder.call                              (models/encoders/rnnt.py:181-186)   Reshape -> blocks
         RnnTransducerBlock.call                                (:73-85)   [TimeReduction] -> LSTM -> [LayerNormalization] -> Dense -> [TimeReduction]
         TimeReduction.call                                     (models/layers/subsampling.py:34-40)
         math_util.get_reduced_length                           (utils/math_util.py:82-89)   ceil(length / factor)

    features [B, T, F, 1] -> Reshape [B, T, F] -> per block:
        pre:   zero-pad T to a multiple of f, view [B, T / f, f * w], lengths ceil(len / f)
        LSTM(rnn_units, zero_output_for_mask) -> LayerNormalization(rnn_units) -> Dense(dmodel)
        post:  the same reduction on the projected rows

Per block: one tfasr_gemm for the LSTM's input projection (for a `pre` block on the reduced VIEW of the rows in front of it),
tfasr_lstm_infer_fwd with the block's lengths, and the block tail into a buffer [B, Tpad, dmodel] with Tpad a multiple of this block's
`post` factor times the next block's `pre` factor, so both reductions are views.  The tail has two routes (`tail_route`).  "fused" is
tfasr_rnnt_block_tail_fwd (csrc/rnnt_block.hip): LayerNorm + Dense in one launch that also writes the zero rows tf.pad would add, the
reduced lengths and, in a streaming step, each stream's rows behind its carried rows; the normalised [rows, rnn_units] activation never
reaches HBM.  "unfused" is tfasr_layernorm_fwd + tfasr_gemm into the padded buffer + a zero fill of the pad rows; it is also the route
of encoder_layer_norm False (the class default: the tail is the Dense alone) and of a width outside the kernel's range.  "auto", the
default, is the unfused route: measured, the one launch is not the faster one in either type (see tail_route below).

Masking is the reference's.  The LSTM emits zeros at frames >= length; LayerNormalization turns a zero row into beta and the Dense
into beta . W + bias, so masked rows are NOT zero behind a block - and a `post` reduction groups them with valid rows: in the last
reduced frame of a shorter batch row the group mixes valid frames with beta . W + bias rows where the utterance run alone has tf.pad's
zeros.  A padded batch row is therefore NOT the utterance alone (the reference's own classes pin this: tests/golden/rnnt_wiring.npz).

The prediction and joint networks, the decoders (greedy, host and device beam search, n-best), forced alignment, evaluate, the precision
switch (f32 twin by default, bf16 opt-in) and the .npz checkpoints are TransducerModel's / AsrModel's; time_reduction_factor is the product of
the blocks' factors.  A `post` reduction in the LAST block widens the encoder's output rows to factor * dmodel (cfg.dmodel), on which the
joint network's encoder projection is built, as keras builds it.

Streaming.  stream() / stream_state() / encode_chunk() open the session of the other causal models (streaming.StreamingRecognizer,
RnntStreamState, rnnt_encode_chunk).  Carried per stream: every block's LSTM (h, c) - the reference's call_next states, in its layout:
RnntStreamState.reference_states() is [B, nlayers, 2, rnn_units] - and, in front of every reduction, the fewer-than-factor rows that do
not fill a group yet with their count.  A step puts each stream's new rows behind its carried rows (the fused tail through its row
offset, the unfused one through a gather), whole groups go on, and finish() fills a stream's last group with zero rows as tf.pad does offline.  This is NOT what the
reference's call_next computes (encoders/rnnt.py:92-121, 188-211): that pads every chunk to whole groups on its own, so its chunked
output equals its offline output only for chunks of whole groups.

Training, GRU / SimpleRNN, more than one prediction LSTM, the prediction
projection and .weights.h5 import are not built: train_step / loss_and_backward / compile raise.
"""
import torch

from . import kernels as K
from .inference_only import InferenceOnlyEncoder
from .params import rnnt_modules
from .transducer import TransducerModel

_LN_EPS = 1e-3  # keras.layers.LayerNormalization default


def _round_up(n, m):
    return -(-int(n) // m) * m


def boundary_factors(mods):
    """The time reductions per block BOUNDARY of rnnt_modules(cfg): [pre_0, post_0 * pre_1, ..., post_{L-1}].  A `post` reduction by f
    followed by the next block's `pre` reduction by g groups f g consecutive rows (zero rows pad either; no layer sits between them)."""
    pre = [m["factor"] if m["position"] == "pre" else 1 for m in mods]
    post = [m["factor"] if m["position"] == "post" else 1 for m in mods]
    return [pre[0]] + [post[i] * pre[i + 1] for i in range(len(mods) - 1)] + [post[-1]]


class RnnEncoderMixin(InferenceOnlyEncoder):
    """encoder_fwd and what it needs; mixed in front of TransducerModel"""

    encoder_kind = "rnnt"
    _not_built = "the encoder's LSTM and block-tail gradients are not built"

    # "fused": tfasr_rnnt_block_tail_fwd; "unfused": tfasr_layernorm_fwd + tfasr_gemm + the zero fill; "auto": the faster of the two as
    # measured (profiles/rnnt_timing.json, small config, 32 x 10 s) - which is the two launches in BOTH types: on layer 0's rows the one
    # launch takes 0.095 against 0.089 ms in bf16 and, a plain FMA kernel, 0.68 against 0.38 ms in f32; a block, the encoder and
    # `recognize` do not tell the routes apart (the recurrence is 99 % of them), a session step is 3 - 6 % slower on the one launch
    tail_route = "auto"

    def _init_encoder(self):
        super()._init_encoder()
        self.modules = rnnt_modules(self.cfg)

    # ------------------------------------------------------------------------------------------- streaming (tensorflowasr_amd/streaming.py)
    def stream(self, batch_size=1, chunk_frames=32, beam_width=0, max_frames=3000, precision=None, max_tokens_per_frame=3):
        """Incremental recognition session (streaming.StreamingRecognizer) over steps of `chunk_frames` feature frames (any positive
        number: rows that do not fill a reduction's group yet are carried).  Stream b holds, bit for bit, the frames `encode` gives that
        utterance alone and the tokens `recognize` gives it, however the samples arrive and whatever the other streams do.  Sessions,
        beams and their memory as ConformerTransducer.stream."""
        from . import streaming

        return streaming.StreamingRecognizer(self, batch_size, precision, max_tokens_per_frame, beam_width, max_frames, chunk_frames=chunk_frames)

    def boundary_factors(self):
        return boundary_factors(self.modules)

    # ------------------------------------------------------------------------------------------- constants derived from the weights
    def _fused_tail(self, m):
        route = self.tail_route
        if route == "auto":
            route = "unfused"
        if not m["ln"] or route == "unfused":
            return False
        ok = K.rnnt_block_tail_supported(m["P"], m["dout"])
        if self.tail_route == "fused" and not ok:
            raise K._lib.TfasrUnsupported(f"{m['name']}: rnn_units {m['P']} x dmodel {m['dout']} is outside tfasr_rnnt_block_tail_fwd's range")
        return ok

    def _projection(self, m):
        """the Dense kernel as the tail reads it: the f32 Keras kernel, or (bf16, fused route) the packed copy"""
        name = m["name"] + "/projection/w"
        if self.dtype == torch.float32 or not self._fused_tail(m):
            return self.ps.w2d(name)
        d = self._cache()
        got = d.get((name, "packed"))
        if got is None:
            got = d[(name, "packed")] = K.conv1d_pack_weight(self.ps.p(name).view(1, m["P"], m["dout"]))
        return got

    # ------------------------------------------------------------------------------------------- encoder
    def lstm_fwd(self, x, m, lens_dev):
        """the LSTM of one block: x [B, T, Din] -> [B, T, P], zeros at frames >= lens"""
        ps, p = self.ps, m["name"] + "/lstm"
        B, T, Din = x.shape
        xg = K.matmul(x.reshape(B * T, Din), ps.w2d(p + "/k"), bias=ps.p(p + "/b")).view(B, T, 4 * m["P"])
        return K.lstm_infer_fwd(xg, ps.w(p + "/rk").view(1, m["P"], 4 * m["P"]), lens_dev)

    def tail_fwd(self, y, m, lens_dev, Tpad, factor, off=None, out=None):
        """LayerNormalization + Dense of one block over y [B, T, P] -> (out [B, Tpad, dmodel], lengths [B] int32 = ceil((off + len) /
        factor)): rows [off + T, Tpad) zero, masked rows computed from zeros.  Tpad % factor == 0."""
        ps, p = self.ps, m["name"]
        B, T, P = y.shape
        N = m["dout"]
        bias = ps.p(p + "/projection/b")
        if self._fused_tail(m):
            return K.rnnt_block_tail_fwd(y, ps.p(p + "/ln/g"), ps.p(p + "/ln/b"), self._projection(m), bias, N, lengths=lens_dev, off=off,
                                         factor=factor, Tpad=Tpad, out=out, eps=_LN_EPS)
        if off is not None:
            raise K._lib.TfasrUnsupported(f"{p}: a row offset needs the fused tail (tfasr_rnnt_block_tail_fwd)")
        # the two-launch route: the masked rows of y are the LSTM's zeros already
        if out is None:
            out = torch.empty(B, Tpad, N, dtype=y.dtype, device=y.device)
        if m["ln"]:
            y = K.layernorm_fwd(y, ps.p(p + "/ln/g"), ps.p(p + "/ln/b"), eps=_LN_EPS, save_stats=False)[0]
        if T:
            K.gemm(y, ps.w2d(p + "/projection/w"), out, T, N, P, P, N, N, bias=bias, nb1=B, sA=(T * P, 0), sD=(Tpad * N, 0))
        if Tpad > T:
            out[:, T:].zero_()
        lens = torch.div(torch.clamp(lens_dev, 0, T) + (factor - 1), factor, rounding_mode="floor").to(torch.int32)
        return out, lens

    def reduce_pre(self, x, T, f):
        """TimeReduction in front of a block: x [B, Tp >= T, w] whose rows at and past T are zero -> the view [B, ceil(T / f), f * w]
        (a copy into a zero-padded buffer when Tp is no multiple of f: the features of block 0)"""
        B, Tp, w = x.shape
        Tr = -(-T // f)
        if Tp != Tr * f:
            pad = torch.zeros(B, Tr * f, w, dtype=x.dtype, device=x.device)
            pad[:, :T].copy_(x[:, :T])
            x = pad
        return x.view(B, Tr, f * w), Tr

    def encoder_fwd(self, feats, flen, training, ctx):
        """RnnTransducerEncoder.call (encoders/rnnt.py:181-186): features [B, T0, F] -> [B*T', cfg.dmodel], T', lengths (host), lengths
        (device)."""
        if training or ctx is not None:
            self._inference_only()
        mods = self.modules
        B, T = feats.shape[:2]
        x = feats.contiguous()
        lens = [min(max(int(n), 0), T) for n in flen]
        lens_dev = self._h2d(lens)
        for i, m in enumerate(mods):
            f = m["factor"]
            pre, post = m["position"] == "pre" and f > 1, m["position"] == "post" and f > 1
            if pre:
                x, T = self.reduce_pre(x, T, f)
                if i == 0:  # (behind a block the tail has written the reduced lengths already)
                    lens = [-(-n // f) for n in lens]
                    lens_dev = self._h2d(lens)
            y = self.lstm_fwd(x, m, lens_dev)
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            g = nxt["factor"] if nxt is not None and nxt["position"] == "pre" else 1
            fp = f if post else 1
            Tpad = _round_up(T, fp * g)
            x, lens_dev = self.tail_fwd(y, m, lens_dev, Tpad, fp * g)
            lens = [-(-n // (fp * g)) for n in lens]
            if post:
                x, T = x.view(B, Tpad // f, f * m["dout"]), -(-T // f)
        # (a `pre` reduction of a block that does not exist cannot be pending here: g = 1 for the last block)
        return x.reshape(B * T, x.shape[2]), T, lens, lens_dev


class RnnTransducer(RnnEncoderMixin, TransducerModel):
    _config_error = "RnnTransducer needs an RnnTransducerConfig (configs.rnnt() / configs.rnnt_from_reference(mapping))"
