"""Jasper CTC model (BASELINE.json configs[4]) on the HIP kernels and C ABI of the other models, inference only.

Mirrors  tensorflow_asr.models.ctc.jasper.Jasper            (models/ctc/jasper.py:61-126: JasperEncoder + JasperDecoder)
         JasperEncoder.call                                  (models/encoders/jasper.py:322-334)
         JasperSubBlock / JasperResidual / JasperSubBlockResidual.call   (:61-67, :102-105, :152-161)
         JasperDecoder: Conv1D(vocab_size, 1) "logits"       (models/ctc/jasper.py:23-48) = the Dense decoder's GEMM

    encoder = reshape [B,T,F,1] -> [B,T,F]; first_block; blocks with the running residual list; second_block; third_block
    sub-block = Conv1D(causal) -> BatchNormalization -> ReLU
    last sub-block of a block = Conv1D -> BatchNormalization -> + sum_r BatchNormalization_r(pointwise_r(residual_r)) -> ReLU

Every layer is one launch of tfasr_conv1d_fwd (csrc/conv1d.hip): the inference BatchNorm (moving statistics, keras epsilon 1e-3) is folded
once per weight load, in f32, to scale = gamma / sqrt(var + eps), shift = beta - mean * scale, applied in the kernel's epilogue with the
bias; a residual branch is the same entry point with one tap, no ReLU and the running sum as `addend`, and the block's main convolution
takes that sum as its addend with the ReLU on.  bf16 models read a packed bf16 copy of each kernel made at the same time; the cache is
dropped whenever the parameter store's weights change (load_weights, import_keras).

Padded frames need no masking: every layer is causal and the BatchNorm is affine, so frame t of an utterance depends on its frames <= t
only - what lies behind an utterance's end in a batch row cannot reach a valid frame, and a batch row equals the utterance run alone.

The front end, the CTC decoders (greedy, host and device beam search, n-best), forced alignment, evaluate, the precision switch (f32
twin by default, bf16 opt-in) and the .npz checkpoints are CtcModel's / AsrModel's.  The feature logarithm is base 10 where the config says so
(speech_config.log_base, feature_extraction.py:214-218): the natural-log features times 1 / ln 10.  Training (Conv1D gradients,
BatchNorm batch statistics) is not built: train_step / loss_and_backward / compile raise.
"""
import math

import torch

from . import kernels as K
from .ctc_model import CtcModel
from .inference_only import InferenceOnlyEncoder
from .params import jasper_modules


class JasperEncoderMixin(InferenceOnlyEncoder):
    """the front end in the config's log base, encoder_fwd and the streaming session; mixed in front of CtcModel"""

    encoder_kind = "jasper"
    _not_built = "the Conv1D data / weight gradients and BatchNorm in batch-statistics mode are not built"

    def _init_encoder(self):
        super()._init_encoder()
        self.layers = jasper_modules(self.cfg)

    # ------------------------------------------------------------------------------------------- constants derived from the weights
    def _layer_consts(self, conv, bn):
        """(kernel in the compute type's layout, bias, scale, shift) of one Conv1D + BatchNormalization pair"""
        ps, d = self.ps, self._cache()
        key = (conv, self.dtype)
        got = d.get(key)
        if got is None:
            aff = self._affine(bn)
            w = ps.p(conv + "/w")
            if self.dtype != torch.float32:
                w = K.conv1d_pack_weight(w)
            got = d[key] = (w, ps.p(conv + "/b"), aff[0], aff[1])
        return got

    def _conv(self, x, conv, bn, shape, stride=1, dilation=1, addend=None, relu=True, lead=0):
        w, bias, scale, shift = self._layer_consts(conv, bn)
        return K.conv1d_fwd(x, w, shape, bias=bias, scale=scale, shift=shift, addend=addend, relu=relu, stride=stride, dilation=dilation,
                            lead=lead)

    def _layer_fwd(self, x, m, residuals, lead=0):
        """One module of jasper_modules: x [B, lead + T, Cin] -> [B, ceil(T / stride), Cout]; residuals = the running list [B, T', C_r]."""
        add = None
        for rname, rcin, src in m["residuals"] or []:
            add = self._conv(residuals[src], rname + "/pointwise_conv1d", rname + "/bn", (1, rcin, m["cout"]), addend=add, relu=False)
        return self._conv(x, m["name"] + "/conv1d", m["name"] + "/bn", (m["K"], m["cin"], m["cout"]), m["stride"], m["dilation"], addend=add,
                          relu=True, lead=lead)

    # ------------------------------------------------------------------------------------------- front end + encoder
    def _scale_feats(self, feats32):
        """natural-log mel features (f32) -> the config's log base, in the compute type"""
        if self.cfg.log_base == "10":
            y = torch.zeros_like(feats32)
            K.axpy(y, feats32, 1.0 / math.log(10.0))
            feats32 = y
        if self.dtype != torch.float32:
            feats32 = K.cast(feats32, torch.empty(feats32.shape, dtype=self.dtype, device=feats32.device))
        return feats32

    def _features(self, signals, signals_length):
        c = self.cfg
        window, melw, band = self._frontend_consts()
        feats = K.logmel(signals, window, melw, band, c.frame_step, c.nfft, c.preemphasis, c.epsilon, torch.float32)
        return self._scale_feats(feats), [-(-int(n) // c.frame_step) for n in signals_length]

    def encoder_fwd(self, feats, flen, training, ctx):
        """JasperEncoder.call (encoders/jasper.py:322-334): features [B, T0, F] -> [B*T', dmodel], T', lengths."""
        if training or ctx is not None:
            self._inference_only()
        B = feats.shape[0]
        x, residuals, starts = feats.contiguous(), [], self._block_starts()
        for li, m in enumerate(self.layers):
            if li in starts:
                residuals.append(x)  # JasperBlock.call:215-219 (not dense: the module reads its own block's entry only)
            x = self._layer_fwd(x, m, residuals)
        T = x.shape[1]
        lens = [self.cfg.encoder_length(n) for n in flen]
        return x.view(B * T, self.cfg.dmodel), T, lens, self._h2d(lens)

    def _block_starts(self):
        """indices into self.layers of every block's first sub-block (whose input joins the residual list)"""
        n = int(self.cfg.nsubblocks)
        return {1 + i * n for i in range(len(self.cfg.block_channels))}

    # ------------------------------------------------------------------------------------------- streaming
    def stream(self, batch_size=1, chunk_frames=32, beam_width=0, max_frames=3000, precision=None):
        """Incremental recognition session (streaming.StreamingRecognizer) over steps of `chunk_frames` feature frames (even: the first
        block strides by 2).  Jasper is causal throughout, so a stream carries only the last (K - 1) * dilation input rows of every layer
        with more than one tap, and holds bit for bit the frames `encode` gives the utterance alone.  beam_width as ConformerCTC's."""
        from . import streaming

        return streaming.StreamingRecognizer(self, batch_size, precision, 1, beam_width, max_frames, chunk_frames=chunk_frames)


class JasperCTC(JasperEncoderMixin, CtcModel):
    _config_error = "JasperCTC needs a JasperConfig (configs.jasper() / configs.jasper_from_reference(mapping))"
