"""DeepSpeech2 CTC model (BASELINE.json configs[0]) on the HIP kernels and C ABI of the other models, inference only.

Mirrors  tensorflow_asr.models.ctc.deepspeech2.DeepSpeech2  (models/ctc/deepspeech2.py:57-130: DeepSpeech2Encoder + DeepSpeech2Decoder)
         DeepSpeech2Encoder.call                             (models/encoders/deepspeech2.py:498-503)
         ConvBlock.call / compute_mask                       (:105-133)   Conv2D -> BatchNormalization -> ReLU, lengths over the time stride
         RnnBlock.call                                       (:250-256)   [Bidirectional] LSTM(zero_output_for_mask) [-> RowConv1D]
         RowConv1D.call                                      (:56-60)     causal DepthwiseConv1D (no bias) -> BatchNormalization -> ReLU
         FcBlock.call                                        (:367-372)   Dense -> ReLU
         DeepSpeech2Decoder: Dense(vocab_size) "logits"      (models/ctc/deepspeech2.py:22-44)

    features [B, T, F, 1] -> conv blocks -> [B, T', F', C] -> Reshape (merge_two_last_dims: the channels-last buffer as it lies,
    column f * C + c) -> per RnnBlock one GEMM for the input projections of all directions + one tfasr_lstm_infer_fwd -> FC blocks

Every conv block is one launch of tfasr_conv2d_fwd (csrc/conv2d_gen.hip): the inference BatchNorm (moving statistics, keras epsilon 1e-3)
is folded once per weight load, in f32, to scale = gamma / sqrt(var + eps), shift = beta - mean * scale and applied in the kernel's
epilogue with the bias and the ReLU.  A Bidirectional layer's two kernels lie side by side in one [Din, 8P] matrix, so its input
projection is one GEMM and the recurrence one call (csrc/lstm_infer.hip: one persistent launch over both directions in bf16, the
per-step kernels otherwise); direction d writes columns [d P, (d + 1) P) of the output, which is the concat merge.  An FC block is
tfasr_conv1d_fwd with one tap (bias + ReLU in its epilogue).  bf16 models read packed / concatenated bf16 copies made at the same time;
the cache is dropped whenever the parameter store's weights change.

Masking.  The mask every LSTM sees is sequence_mask(conv-reduced length) (ConvBlock.compute_mask, carried through Reshape and each
RnnBlock): frames at or past it carry the state and emit zeros.  Nothing else is masked, as in the reference: with "same" padding the
convolutions of a short utterance's last valid frames read the padded tail of its batch row - whose features are ln(epsilon), not 0 - and
the backward LSTM direction starts from them.  A batch row of the base ("same", bidirectional) config is therefore NOT the utterance run
alone; that is the reference's behaviour on a padded batch and is reproduced, not masked away.  The causal unidirectional variant has no
such path: there a batch row equals the utterance alone.

The CTC decoders (greedy, host and device beam search, n-best), forced alignment, evaluate, the precision switch (f32 twin by default,
bf16 opt-in) and the .npz checkpoints are CtcModel's / AsrModel's.  feature_type "spectrogram" (feature_extraction.py:233-235: ln(|STFT|^2 + eps),
first num_feature_bins bins) runs on the log-mel kernel with the first F columns of the identity as its weight matrix.  Training,
GRU / SimpleRNN, conv_type conv1d and .weights.h5 import are not built: train_step / loss_and_backward / compile raise.

Streaming.  A config that is causal throughout (conv_padding "causal", rnn_bidirectional False: uni.yml.j2) opens the session of the
other causal models: stream() / stream_state() / encode_chunk() (streaming.StreamingRecognizer, DS2StreamState, ds2_encode_chunk).
Stream b holds, bit for bit, the encoder frames `encode` gives that utterance alone and the tokens `recognize` gives it, however the
samples arrive and whatever the other streams do.  Carried per stream: the last kh - 1 input rows of every conv block, each LSTM's
(h, c) and the last K - 1 input rows of every RowConv1D.  This is NOT what the reference's DeepSpeech2Encoder.call_next computes
(encoders/deepspeech2.py:505-524): that carries the LSTM states only and runs the conv module and every RowConv1D on each chunk with
fresh causal zero padding, so its chunked output differs from its own offline output in the first kh - 1 encoder frames of every chunk
and in the 2w frames behind them in every RowConv1D.  The LSTM states carried here are the reference's, in its layout:
DS2StreamState.reference_states() is [B, nlayers, 2, P], (h, c), what get_initial_state / call_next exchange.  Any other config
(bidirectional, "same" padding) refuses all three calls with the reason, before it looks at an argument.
"""
import numpy as np
import torch

from . import kernels as K
from .ctc_model import CtcModel
from .inference_only import InferenceOnlyEncoder
from .params import deepspeech2_modules


class DeepSpeech2EncoderMixin(InferenceOnlyEncoder):
    """the front end (log-mel or spectrogram), encoder_fwd and the causal variant's streaming session; mixed in front of CtcModel"""

    encoder_kind = "deepspeech2"
    _not_built = "the Conv2D / LSTM gradients and BatchNorm in batch-statistics mode are not built"

    def _init_encoder(self):
        super()._init_encoder()
        self.modules = deepspeech2_modules(self.cfg)

    # ------------------------------------------------------------------------------------------- streaming (the causal variant)
    def stream(self, batch_size=1, chunk_frames=32, beam_width=0, max_frames=3000, precision=None):
        """Incremental recognition session (streaming.StreamingRecognizer) over steps of `chunk_frames` feature frames, a positive multiple
        of the product of the time strides.  Only a config that is causal throughout streams (see the module docstring); a stream then
        holds bit for bit the frames `encode` gives the utterance alone.  beam_width as ConformerCTC's."""
        from . import streaming

        streaming.check_streamable(self)
        return streaming.StreamingRecognizer(self, batch_size, precision, 1, beam_width, max_frames, chunk_frames=chunk_frames)

    # ------------------------------------------------------------------------------------------- constants derived from the weights
    def _conv_consts(self, name):
        d, ps = self._cache(), self.ps
        got = d.get((name, self.dtype))
        if got is None:
            w = ps.p(name + "/conv2d/w")
            if self.dtype != torch.float32:
                w = K.conv2d_pack_weight(w)
            got = d[(name, self.dtype)] = (w, ps.p(name + "/conv2d/b"), *self._affine(name + "/bn"))
        return got

    def _rnn_consts(self, r):
        """(kernels of the directions side by side [Din, ndir * 4P], biases [ndir * 4P] f32, recurrent kernels [ndir, P, 4P])"""
        d, ps = self._cache(), self.ps
        got = d.get((r["name"], self.dtype))
        if got is None:
            k = torch.cat([ps.w(x + "/k") for x in r["dirs"]], dim=1).contiguous()
            b = torch.cat([ps.p(x + "/b") for x in r["dirs"]]).contiguous()
            rk = torch.stack([ps.w(x + "/rk") for x in r["dirs"]]).contiguous()
            got = d[(r["name"], self.dtype)] = (k, b, rk)
        return got

    def _fc_consts(self, f):
        d, ps = self._cache(), self.ps
        got = d.get((f["name"], self.dtype))
        if got is None:
            w = ps.p(f["name"] + "/fc/w").view(1, f["din"], f["dout"])
            if self.dtype != torch.float32:
                w = K.conv1d_pack_weight(w)
            got = d[(f["name"], self.dtype)] = (w, ps.p(f["name"] + "/fc/b"))
        return got

    # ------------------------------------------------------------------------------------------- front end
    def _frontend_consts(self):
        if self.cfg.feature_type != "spectrogram":
            return super()._frontend_consts()
        if "fe" not in self._consts:
            c = self.cfg
            n, F, bins = c.frame_length, int(c.num_feature_bins), c.nfft // 2 + 1
            window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(np.float32)  # periodic Hann
            melw, band = spectrogram_weights(F, bins)
            dev = self.device
            self._consts["fe"] = (torch.from_numpy(window).to(dev), torch.from_numpy(melw).to(dev), torch.from_numpy(band).to(dev))
        return self._consts["fe"]

    def _features(self, signals, signals_length):
        c = self.cfg
        window, melw, band = self._frontend_consts()
        feats = K.logmel(signals, window, melw, band, c.frame_step, c.nfft, c.preemphasis, c.epsilon, torch.float32)
        if self.dtype != torch.float32:
            feats = K.cast(feats, torch.empty(feats.shape, dtype=self.dtype, device=feats.device))
        return feats, [-(-int(n) // c.frame_step) for n in signals_length]

    # ------------------------------------------------------------------------------------------- encoder
    def conv_module_fwd(self, feats):
        """features [B, T, F] -> [B, T', F', C] (ConvModule.call :185-190 without the final Reshape)"""
        x = feats.contiguous().view(*feats.shape, 1)
        for m in self.modules["convs"]:
            w, bias, scale, shift = self._conv_consts(m["name"])
            x = K.conv2d_fwd(x, w, (m["kh"], m["kw"], m["cin"], m["cout"]), bias=bias, scale=scale, shift=shift, relu=True,
                             strides=(m["st"], m["sf"]), padding=self.cfg.conv_padding)
        return x

    def lstm_fwd(self, x, r, lens_dev):
        """the [Bidirectional] LSTM of one RnnBlock: x [B, T', Din] -> [B, T', ndir * P], zeros at frames >= lens"""
        B, T, Din = x.shape
        k, b, rk = self._rnn_consts(r)
        xg = K.matmul(x.view(B * T, Din), k, bias=b).view(B, T, k.shape[1])
        return K.lstm_infer_fwd(xg, rk, lens_dev, ndir=len(r["dirs"]))

    def rnn_block_fwd(self, x, r, lens_dev):
        """one RnnBlock (LSTM [-> RowConv1D]): x [B, T', Din] -> [B, T', ndir * P]"""
        y = self.lstm_fwd(x, r, lens_dev)
        if r["rowconv"]:
            scale, shift = self._affine(r["rowconv"] + "/bn")
            y = K.dwconv_fwd(y, self.ps.p(r["rowconv"] + "/conv/w"), None)
            y = K.channel_affine_fwd(y, scale, shift, relu=True)
        return y

    def encoder_fwd(self, feats, flen, training, ctx):
        """DeepSpeech2Encoder.call (encoders/deepspeech2.py:498-503): features [B, T0, F] -> [B*T', dmodel], T', lengths."""
        if training or ctx is not None:
            self._inference_only()
        x = self.conv_module_fwd(feats)
        B, T = x.shape[:2]
        lens = [self.cfg.encoder_length(n) for n in flen]
        lens_dev = self._h2d(lens)
        x = x.view(B, T, -1)
        for r in self.modules["rnns"]:
            x = self.rnn_block_fwd(x, r, lens_dev)
        for f in self.modules["fcs"]:
            w, bias = self._fc_consts(f)
            x = K.conv1d_fwd(x, w, (1, f["din"], f["dout"]), bias=bias, relu=True)
        return x.view(B * T, self.cfg.dmodel), T, lens, lens_dev


class DeepSpeech2CTC(DeepSpeech2EncoderMixin, CtcModel):
    _config_error = "DeepSpeech2CTC needs a DeepSpeech2Config (configs.deepspeech2() / configs.deepspeech2_from_reference(mapping))"


def spectrogram_weights(F, bins=257):
    """(melw [bins, F], band [F, 2]) that make the log-mel kernel emit ln(|STFT|^2 + eps)[:, :, :F]: the first F columns of the identity,
    band[f] = (f, f)."""
    melw = np.zeros((bins, F), np.float32)
    melw[np.arange(F), np.arange(F)] = 1.0
    band = np.stack([np.arange(F), np.arange(F)], 1).astype(np.int32)
    return melw, band
