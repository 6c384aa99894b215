"""Conformer-CTC on the same HIP kernels and C ABI as the transducer path.

Mirrors  tensorflow_asr.models.ctc.conformer.Conformer      (models/ctc/conformer.py:57-143: ConformerEncoder + ConformerDecoder)
         ConformerDecoder.call                              (models/ctc/conformer.py:21-47: one Dense(vocab_size) named "logits")
         CtcModel.call / recognize / recognize_beam         (models/ctc/base_ctc.py:74-149)
         CtcLoss.call                                       (losses/ctc_loss.py:47-66: tf.nn.ctc_loss, blank 0, mean over the batch)

CtcModel is the CTC head over any encoder (model.AsrModel's docstring): the Dense decoder and tfasr_ctc_loss with a hand-written backward
around encoder_fwd / encoder_bwd; the log-mel frontend, SpecAugment, optimizer, gradient accumulation and the data-parallel hooks are
AsrModel's, the subsampling and the Conformer blocks (native block executor) ConformerEncoderMixin's.  Decoding: tfasr_ctc_greedy_decode
(device) and tfasr_ctc_beam_search_host (host routine, as tf.nn.ctc_beam_search_decoder is; the default of recognize_beam) or
tfasr_ctc_beam_search (the same search on the device, with the n-best list: recognize_beam(device_search=True), recognize_nbest).
No CPU fallback.
"""
import torch

from . import kernels as K
from .conformer import ConformerEncoderMixin
from .model import AsrModel
from .schemas import AlignOutput, NBestOutput, PredictInput, PredictOutput, RecognizeOutput, TrainData, TrainInput, TrainOutput


class CtcModel(AsrModel):
    head_kind = "ctc"

    def get_initial_decoder_states(self, batch_size=1):
        return None  # a CTC decoder carries nothing from call to call (the decoders' call_next return None, models/ctc/deepspeech2.py:129-130)

    # ------------------------------------------------------------------------------------------- forward
    def _forward_ctc(self, inputs: TrainInput, training, ctx, masks=None):
        dev = self.device
        self._drop_epoch += 1
        sig = inputs.inputs.to(dev, non_blocking=True)
        slen = [int(v) for v in inputs.inputs_length.tolist()]
        feats, flen = self.frontend(sig, slen, training, masks)
        enc, T, elen, elen_dev = self.encoder_fwd(feats, flen, training, ctx)
        ps = self.ps
        B = sig.shape[0]
        logits = K.matmul(enc, ps.w2d("dec/logits/w"), bias=ps.p("dec/logits/b")).view(B, T, self.cfg.vocab_size)
        if ctx is not None:
            ctx["dec"] = dict(enc=enc, B=B, T=T)
        return logits, elen, elen_dev

    def __call__(self, inputs: TrainInput, training=False):
        """CtcModel.call (base_ctc.py:74-81)."""
        logits, elen, _ = self._forward_ctc(inputs, training, None)
        return TrainOutput(logits=logits, logits_length=torch.tensor(elen, dtype=torch.int32))

    # ------------------------------------------------------------------------------------------- loss + backward
    def loss_and_backward(self, data: TrainData, training=True, masks=None, want_backward=True, packed=True, reduce=True):
        """forward, CtcLoss (mean over the batch) and the full backward into the flat gradient buffer (accumulating)."""
        self.dp.set_reduce(bool(reduce))
        ctx = {} if want_backward else None
        dev = self.device
        logits, elen, elen_dev = self._forward_ctc(data.inputs, training, ctx, masks)
        B, T, V = logits.shape
        labels = data.labels.labels.to(dev, non_blocking=True).to(torch.int32).contiguous()
        llen = [int(v) for v in data.labels.labels_length.tolist()]
        # BaseLoss.call: logit_length = max(logit_length, label_length)  (losses/base_loss.py:36), bounded by the padded length
        tl = [min(max(int(a), b), T) for a, b in zip(elen, llen)]
        tl_dev, ul_dev = self._h2d(tl), self._h2d(llen)
        gscale = torch.full((B,), 1.0 / (B * self.dp.world), dtype=torch.float32, device=dev)
        costs, dlogits = K.ctc_loss_fwd_bwd(logits, labels, ul_dev, tl_dev, grad_scale=gscale, grads=logits, want_grads=want_backward,
                                            blank=self.blank)
        if not want_backward:
            return costs
        s = ctx["dec"]
        denc = self._dense_bwd(dlogits.view(B * T, V), s["enc"], "dec/logits/w", "dec/logits/b")
        self.dp.grads_ready(self.ps.offsets["dec/logits/w"], self.ps.n_reg)
        self.encoder_bwd(denc, ctx)
        self.dp.finish_grads()
        return costs

    # ------------------------------------------------------------------------------------------- decoding
    @torch.no_grad()
    def _infer_logits(self, inputs: PredictInput):
        enc, elen = self.encode(inputs.inputs, inputs.inputs_length)
        B, T, d = enc.shape
        ps = self.ps
        # decision arithmetic in f32 on the f32 master weights (the reference's greedy / beam decoders read f32 logits)
        enc32 = enc.reshape(B * T, d)
        if enc32.dtype != torch.float32:
            enc32 = K.cast(enc32.contiguous(), torch.empty(B * T, d, dtype=torch.float32, device=self.device))
        logits = K.matmul(enc32, ps.p2d("dec/logits/w"), bias=ps.p("dec/logits/b")).view(B, T, self.cfg.vocab_size)
        return logits, elen

    @torch.no_grad()
    def recognize(self, inputs: PredictInput, **kwargs):
        """CtcModel.recognize (base_ctc.py:102-124): tf.nn.ctc_greedy_decoder(merge_repeated=True, blank_index=blank), dense, 0 padded."""
        logits, elen = self._infer_logits(inputs)
        tokens, tlen = K.ctc_greedy_decode(logits, self._h2d(elen), blank=self.blank)
        width = max(int(tlen.max().item()), 1)  # tf.sparse.to_dense: as wide as the longest decoded sequence
        return PredictOutput(tokens=tokens[:, :width], next_tokens=None, next_encoder_states=None, next_decoder_states=None)

    @torch.no_grad()
    def recognize_detailed(self, inputs: PredictInput, **kwargs):
        """recognize with the span and the confidence of every token (tfasr_ctc_greedy_decode_detail, two launches over the logits of
        _infer_logits) -> RecognizeOutput: token i of utterance b holds the frames [frames[b, i], ends[b, i]) (AlignOutput's definitions),
        log_probs is summed and entropies averaged over them, scores is the log-probability of the best path."""
        logits, elen = self._infer_logits(inputs)
        tokens, tlen, starts, ends, logp, ent, score = K.ctc_greedy_decode_detail(logits, self._h2d(elen), blank=self.blank)
        width = max(int(tlen.max().item()), 1)
        predict = PredictOutput(tokens=tokens[:, :width], next_tokens=None, next_encoder_states=None, next_decoder_states=None)
        return RecognizeOutput(predict, starts[:, :width], ends[:, :width], logp[:, :width], ent[:, :width], score, self.seconds_per_frame,
                               self.cfg.vocab_size)

    @torch.no_grad()
    def recognize_beam(self, inputs: PredictInput, beam_width=10, device_search=False, **kwargs):
        """CtcModel.recognize_beam (base_ctc.py:128-149): tf.nn.ctc_beam_search_decoder(beam_width) - top path, dense.  TF's beam
        search decoder treats the LAST class as blank (the reference does not pass blank_index there): reproduced.
        device_search=True runs the same search on the GPU (tfasr_ctc_beam_search) instead of the host routine."""
        logits, elen = self._infer_logits(inputs)
        if device_search:
            toks, n, _ = K.ctc_beam_search_device(logits, self._h2d(elen), beam_width=beam_width, top_paths=1, blank_index=None)
            toks, n = toks[:, 0], n[:, 0]
        else:
            toks, n, _ = K.ctc_beam_search(logits, torch.tensor(elen, dtype=torch.int32), beam_width=beam_width, blank_index=None)
        width = max(int(n.max().item()), 1)
        return PredictOutput(tokens=toks[:, :width].to(self.device), next_tokens=None, next_encoder_states=None, next_decoder_states=None)

    @torch.no_grad()
    def recognize_nbest(self, inputs: PredictInput, beam_width=10, top_paths=4):
        """n-best list of the beam search (tf.nn.ctc_beam_search_decoder's top_paths), on the GPU: tokens [B, P, T'] (0 padded),
        lengths [B, P], log_prob [B, P], best first; P = top_paths <= beam_width."""
        logits, elen = self._infer_logits(inputs)
        return K.ctc_beam_search_device(logits, self._h2d(elen), beam_width=beam_width, top_paths=top_paths, blank_index=None)

    def _check_lm(self, lm):
        if int(lm.vocab_size) != int(self.cfg.vocab_size) or int(lm.blank) != int(self.blank):
            raise ValueError(f"the language model was built for vocab_size {lm.vocab_size} with blank {lm.blank}; this model has "
                             f"vocab_size {self.cfg.vocab_size} with blank {self.blank}")

    @torch.no_grad()
    def recognize_beam_lm(self, inputs: PredictInput, lm, beam_width=10, alpha=0.5, beta=0.0, device_search=True):
        """The prefix beam search with the n-gram model `lm` (lm.NGramLM) fused in: the top path of argmax_y log P_ctc(y | x) + alpha *
        ln P_lm(y) + beta * |y| (+ alpha * ln P_lm(</s> | y) in the final order), on the GPU (tfasr_ctc_beam_search_lm) or, with
        device_search=False, by the host routine.  1 <= beam_width <= 32.  The blank is the model's own, self.blank - not TF's
        last-class convention that recognize_beam reproduces: there is no reference call to mirror here.  An lm built for another vocabulary size or blank is refused."""
        self._check_lm(lm)
        logits, elen = self._infer_logits(inputs)
        tables = lm.tables(alpha, beta)
        if device_search:
            toks, n = K.ctc_beam_search_lm(logits, self._h2d(elen), tables, beam_width=beam_width, top_paths=1, blank_index=self.blank)[:2]
        else:
            toks, n = K.ctc_beam_search_lm_host(logits, torch.tensor(elen, dtype=torch.int32), tables, beam_width=beam_width, top_paths=1,
                                                blank_index=self.blank)[:2]
        toks, n = toks[:, 0], n[:, 0]
        width = max(int(n.max().item()), 1)
        return PredictOutput(tokens=toks[:, :width].to(self.device), next_tokens=None, next_encoder_states=None, next_decoder_states=None)

    @torch.no_grad()
    def recognize_nbest_lm(self, inputs: PredictInput, lm, beam_width=10, top_paths=4, alpha=0.5, beta=0.0):
        """n-best list of recognize_beam_lm's search, on the GPU: tokens [B, P, T'] (0 padded), lengths [B, P], score [B, P], log_prob
        [B, P] (acoustic), lm_score [B, P], best first by score = log_prob + lm_score; P = top_paths <= beam_width <= 32.  The blank
        is self.blank (see recognize_beam_lm), not TF's last class."""
        self._check_lm(lm)
        logits, elen = self._infer_logits(inputs)
        return K.ctc_beam_search_lm(logits, self._h2d(elen), lm.tables(alpha, beta), beam_width=beam_width, top_paths=top_paths,
                                    blank_index=self.blank)

    @torch.no_grad()
    def recognize_nbest_detailed(self, inputs: PredictInput, beam_width=10, top_paths=4, lm=None, alpha=0.5, beta=0.0):
        """recognize_nbest (or, with `lm`, recognize_nbest_lm) that also says when each token of each hypothesis was spoken and how sure the
        model was -> NBestOutput.  One _infer_logits, the search, then ONE alignment of all B * P hypotheses against the same logits
        (tfasr_ctc_nbest_align: the frame statistics once per utterance, the token array read in place), with the blank the search used:
        the last class for the plain search (TF's convention, see recognize_beam), self.blank with an lm.  `search` is bit for bit what
        recognize_nbest / recognize_nbest_lm return; a path past the last live beam (search score -inf) stays marked: path_scores -inf,
        frames -1.  Columns past TFASR_ALIGN_CTC_MAX_U hold no times."""
        if lm is not None:
            self._check_lm(lm)
        logits, elen = self._infer_logits(inputs)
        elen_dev = self._h2d(elen)
        if lm is None:
            search = K.ctc_beam_search_device(logits, elen_dev, beam_width=beam_width, top_paths=top_paths, blank_index=None)
            blank = self.cfg.vocab_size - 1
        else:
            search = K.ctc_beam_search_lm(logits, elen_dev, lm.tables(alpha, beta), beam_width=beam_width, top_paths=top_paths,
                                          blank_index=self.blank)
            blank = self.blank
        tokens, lengths, score = search[:3]
        live = torch.where(score == float("-inf"), torch.full_like(lengths, -1), lengths)  # dead paths, marked on the device
        start, end, logp, ent, path = K.ctc_nbest_align(logits, elen_dev, tokens, live, blank=blank)
        return NBestOutput(search, tokens, lengths, start, end, logp, ent, path, self.seconds_per_frame, self.cfg.vocab_size)

    @torch.no_grad()
    def align(self, data: TrainData, precision=None):
        """CTC forced alignment of data.labels over the f32 logits of _infer_logits (csrc/align.hip) -> AlignOutput: label u holds the
        frames [frames[b, u], ends[b, u]).  Ties take the smallest move, and the final blank at the end; labels that do not fit their
        frames give score -inf and -1 everywhere."""
        logits, elen = self._infer_logits(PredictInput(data.inputs.inputs, data.inputs.inputs_length))
        B, T, V = logits.shape
        lab = data.labels.labels.to(self.device).to(torch.int32).contiguous()
        tl = [min(max(int(v), 0), T) for v in elen]
        ul = [min(max(int(v), 0), lab.shape[1]) for v in data.labels.labels_length.tolist()]
        start, end, label_lp, score = K.ctc_align(logits, lab, self._h2d(ul), self._h2d(tl), blank=self.blank)
        return AlignOutput(start, end, label_lp, score, self.seconds_per_frame)

    def align_encoded(self, *a, **k):
        raise NotImplementedError("the transducer lattice does not apply to a CTC model: use align")

    def recognize_encoded(self, *a, **k):
        raise NotImplementedError("transducer greedy search does not apply to a CTC model")

    def recognize_encoded_detailed(self, *a, **k):
        raise NotImplementedError("transducer greedy search does not apply to a CTC model")

    def recognize_beam_encoded(self, *a, **k):
        raise NotImplementedError("transducer beam search does not apply to a CTC model")


class ConformerCTC(ConformerEncoderMixin, CtcModel):
    _config_error = "ConformerCTC needs a config with head='ctc' (configs.conformer_ctc_s())"

    def get_initial_decoder_states(self, batch_size=1):
        """As before the heads were split: the zero state of the transducer's prediction LSTM [B, 1, 2, cfg.rnn_units], not the None of
        the other CTC models (the reference's CtcModel returns [], base_ctc.py:97-98)."""
        return torch.zeros(batch_size, 1, 2, self.cfg.rnn_units, dtype=torch.float32, device=self.device)
