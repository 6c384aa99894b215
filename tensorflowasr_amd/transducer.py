"""The transducer head over any encoder: prediction network, joint network, RNN-T loss, greedy / beam search, forced alignment.

Mirrors  Transducer.call / call_next / recognize*                    (models/transducer/base_transducer.py:427-712)
         TransducerPrediction / TransducerJoint                      (base_transducer.py:109-132, 280-293)
         BaseModel._train_step                                       (models/base_model.py:149-183)

The prediction network runs on a second, high-priority HIP stream, overlapped with the encoder (model.AsrModel's docstring: the encoder
calls _side_tick between its blocks).  No CPU fallback.
"""
import os

import numpy as np
import torch

from . import kernels as K
from .kernels import ACT_TANH_OUT
from .model import AsrModel, SingleProcess, _split_k
from .schemas import AlignOutput, NBestOutput, PredictInput, PredictOutput, RecognizeOutput, TrainData, TrainInput, TrainOutput


class TransducerModel(AsrModel):
    head_kind = "transducer"
    aux_stream = None  # an encoder with a side stream of its own sets it (ConformerEncoderMixin); joint_wgrad_aux launches there

    def _init_head(self):
        prio = -1
        self.pred_stream = torch.cuda.Stream(device=self.device, priority=prio)
        self.use_pred_stream = os.environ.get("TFASR_NO_PRED_STREAM", "0") != "1"
        # prediction-network recurrence: the persistent one-launch kernels are faster in isolation but hold P/16 CUs for ~2 ms per step;
        # beside the encoder on the other stream the per-step kernels make the whole step 0.2 ms faster (measured on M and S), so:
        # persistent only when the prediction network has the device to itself.  TFASR_LSTM_PERSIST=0/1 in the environment overrides.
        self._lstm_persist_auto = os.environ.get("TFASR_LSTM_PERSIST") is None
        self.joint_wgrad_aux = False  # (measured no gain: the vocabulary weight gradient on the auxiliary stream)
        self._aux_pending = False
        self.fuse_joint_stats = True
        # Joint + loss WITHOUT materialised lattice logits (SURVEY section 7 step 8 / 8(d) "report both"): the projection emits only the
        # log-softmax statistics, the gradient pass re-computes the logit tile and turns it into the loss gradient in its epilogue
        # (tfasr_gemm_args.rgrad_coef).  Trades two passes over the [cells, V] tensor for one more vocabulary product: measured SLOWER
        # than the materialised route on MI355X (bench.py reports both), so opt-in: TFASR_JOINT_RECOMPUTE=1.
        self.joint_recompute = os.environ.get("TFASR_JOINT_RECOMPUTE", "0") == "1"
        self.decode_fused = True  # the fused search step (4 launches per iteration, queued from C); False: the per-kernel loop (tests)

    # =================================================================================== prediction network
    def prediction_fwd(self, tokens_dev, plen_dev, ctx, h0=None, c0=None):
        """TransducerPrediction.call (base_transducer.py:123-132): Embedding -> LSTM -> LayerNorm. tokens [B,U1] int32."""
        ps, c = self.ps, self.cfg
        B, U1 = tokens_dev.shape
        E, P = c.embed_dim, c.rnn_units
        emb = K.embedding_fwd(tokens_dev, ps.p("pred/emb"), self.dtype).view(B * U1, E)
        xg = K.matmul(emb, ps.w2d("pred/lstm/k"), bias=ps.p("pred/lstm/b")).view(B, U1, 4 * P)
        gates = torch.empty(B, U1, 4 * P, dtype=self.dtype, device=self.device)
        cseq = torch.empty(B, U1, P, dtype=torch.float32, device=self.device)
        hseq = torch.empty(B, U1, P, dtype=self.dtype, device=self.device)
        yseq = torch.empty(B, U1, P, dtype=self.dtype, device=self.device)
        hr = torch.empty(B, 4 * P, dtype=torch.float32, device=self.device)
        Wrk = ps.w2d("pred/lstm/rk")
        if self._lstm_persist_auto:
            K.lstm_set_persist(0 if (self.use_pred_stream and torch.cuda.current_stream(self.device) == self.pred_stream) else 1)
        K.lstm_seq_fwd(xg, Wrk, h0, c0, plen_dev, gates, cseq, hseq, yseq, hr)  # the U1 steps queued from C (one host call)
        y2 = yseq.view(B * U1, P)
        if c.prediction_layer_norm:
            pred, mean, rstd = K.layernorm_fwd(y2, ps.p("pred/ln/g"), ps.p("pred/ln/b"))
        else:  # prediction_layer_norm: False (contextnet/small.yml.j2)
            pred, mean, rstd = y2, None, None
        if ctx is not None:
            ctx["pred"] = dict(tokens=tokens_dev, plen=plen_dev, emb=emb, gates=gates, cseq=cseq, hseq=hseq, y2=y2, mean=mean, rstd=rstd, B=B, U1=U1)
        return pred  # [B*U1, P]

    # ---- the prediction network queued in SLICES between the encoder blocks --------------------------------------------------------------
    # Its recurrence is ~2 x U1 tiny launches per direction on a stream of its own.  Queued in one go, a host that is slower than the GPU
    # (under rocprofv3: tools/prof_streams.py, profiles/r05_streams_single_slices0.txt) blocks in hipLaunchKernel on that stream's full launch
    # queue and starves the ENCODER's stream meanwhile - the main queue idles for the whole duration of the prediction network, once per
    # direction, 21 % of the traced span.  A slice per encoder block keeps both queues fed: traced span 155 -> 128 ms for six steps.
    # Unprofiled the host runs ~3 steps ahead of the GPU (6.5 ms of pure host time per 21.7-ms step), so the gain there is small:
    # 21.75 -> 21.68 ms/step (two interleaved pairs, profiles/r05_dp_queue_sweep.txt).  TFASR_PRED_SLICES=0: in one go.
    def _pred_nslices(self, U1):
        n = int(os.environ.get("TFASR_PRED_SLICES", "8"))
        return max(1, min(n, U1))

    def _prediction_fwd_gen(self, tokens_dev, plen_dev, ctx):
        """prediction_fwd as a generator: every next() queues one slice (on the current stream); the last one sets self._side_result"""
        ps, c = self.ps, self.cfg
        B, U1 = tokens_dev.shape
        E, P = c.embed_dim, c.rnn_units
        emb = K.embedding_fwd(tokens_dev, ps.p("pred/emb"), self.dtype).view(B * U1, E)
        xg = K.matmul(emb, ps.w2d("pred/lstm/k"), bias=ps.p("pred/lstm/b")).view(B, U1, 4 * P)
        gates = torch.empty(B, U1, 4 * P, dtype=self.dtype, device=self.device)
        cseq = torch.empty(B, U1, P, dtype=torch.float32, device=self.device)
        hseq = torch.empty(B, U1, P, dtype=self.dtype, device=self.device)
        yseq = torch.empty(B, U1, P, dtype=self.dtype, device=self.device)
        hr = torch.empty(B, 4 * P, dtype=torch.float32, device=self.device)
        Wrk = ps.w2d("pred/lstm/rk")
        step = -(-U1 // self._pred_nslices(U1))
        for t0 in range(0, U1, step):
            K.lstm_seq_fwd_range(xg, Wrk, None, None, plen_dev, gates, cseq, hseq, yseq, hr, t0, min(U1, t0 + step))
            if t0 + step < U1:
                yield
        y2 = yseq.view(B * U1, P)
        if c.prediction_layer_norm:
            pred, mean, rstd = K.layernorm_fwd(y2, ps.p("pred/ln/g"), ps.p("pred/ln/b"))
        else:
            pred, mean, rstd = y2, None, None
        if ctx is not None:
            ctx["pred"] = dict(tokens=tokens_dev, plen=plen_dev, emb=emb, gates=gates, cseq=cseq, hseq=hseq, y2=y2, mean=mean, rstd=rstd, B=B, U1=U1)
        self._side_result = pred

    def _prediction_bwd_gen(self, dpred, ctx):
        """prediction_bwd as a generator (slices of the backward recurrence in descending time order, then the weight gradients)"""
        ps, c = self.ps, self.cfg
        s = ctx["pred"]
        B, U1 = s["B"], s["U1"]
        E, P = c.embed_dim, c.rnn_units
        if c.prediction_layer_norm:
            dy = K.layernorm_bwd(dpred, s["y2"], ps.p("pred/ln/g"), s["mean"], s["rstd"], ps.g("pred/ln/g"), ps.g("pred/ln/b")).view(B, U1, P)
        else:
            dy = dpred.view(B, U1, P)
        dy = dy.contiguous()
        dz = torch.empty(B, U1, 4 * P, dtype=self.dtype, device=self.device)
        dh_carry = torch.zeros(B, P, dtype=torch.float32, device=self.device)
        dc_carry = torch.zeros(B, P, dtype=torch.float32, device=self.device)
        dhr = torch.empty(B, P, dtype=torch.float32, device=self.device)
        Wrk = ps.w2d("pred/lstm/rk")
        step = -(-U1 // self._pred_nslices(U1))
        t1 = U1
        while t1 > 0:
            t0 = max(0, t1 - step)
            K.lstm_seq_bwd_range(dy, Wrk, s["gates"], s["cseq"], s["plen"], dz, dh_carry, dc_carry, dhr, t0, t1)
            t1 = t0
            yield
        dz2 = dz.view(B * U1, 4 * P)
        if U1 > 1:
            K.gemm(s["hseq"], dz[:, 1:], ps.g2d("pred/lstm/rk"), P, 4 * P, U1 - 1, P, 4 * P, 4 * P, trans_a=True, nb1=B,
                   sA=(U1 * P, 0), sB=(U1 * 4 * P, 0), sD=(0, 0), accumulate=True)
        demb = self._dense_bwd(dz2, s["emb"], "pred/lstm/k", "pred/lstm/b")
        K.embedding_bwd(s["tokens"], demb, ps.g("pred/emb"))

    def _side_tick(self):
        """queue the next slice of the prediction network (if one is pending) on its stream"""
        g = getattr(self, "_side_gen", None)
        if g is None:
            return
        with torch.cuda.stream(self.pred_stream):
            try:
                next(g)
            except StopIteration:
                self._side_gen = None

    def _side_drain(self):
        while getattr(self, "_side_gen", None) is not None:
            self._side_tick()

    def _pred_sliced(self):
        # the per-step kernels are what the overlapped step runs (see _lstm_persist_auto); a forced persistent launch has nothing to slice
        return self.use_pred_stream and self._lstm_persist_auto and os.environ.get("TFASR_PRED_SLICES", "8") != "0"

    def prediction_bwd(self, dpred, ctx):
        ps, c = self.ps, self.cfg
        s = ctx["pred"]
        B, U1 = s["B"], s["U1"]
        E, P = c.embed_dim, c.rnn_units
        if c.prediction_layer_norm:
            dy = K.layernorm_bwd(dpred, s["y2"], ps.p("pred/ln/g"), s["mean"], s["rstd"], ps.g("pred/ln/g"), ps.g("pred/ln/b")).view(B, U1, P)
        else:
            dy = dpred.view(B, U1, P)
        dz = torch.empty(B, U1, 4 * P, dtype=self.dtype, device=self.device)
        dh_carry = torch.zeros(B, P, dtype=torch.float32, device=self.device)
        dc_carry = torch.zeros(B, P, dtype=torch.float32, device=self.device)
        dhr = torch.empty(B, P, dtype=torch.float32, device=self.device)
        Wrk = ps.w2d("pred/lstm/rk")
        if self._lstm_persist_auto:
            K.lstm_set_persist(0 if (self.use_pred_stream and torch.cuda.current_stream(self.device) == self.pred_stream) else 1)
        K.lstm_seq_bwd(dy.contiguous(), Wrk, s["gates"], s["cseq"], s["plen"], dz, dh_carry, dc_carry, dhr)
        dz2 = dz.view(B * U1, 4 * P)
        # recurrent kernel: gR += sum_b h[b, :-1]^T @ dz[b, 1:]
        if U1 > 1:
            K.gemm(s["hseq"], dz[:, 1:], ps.g2d("pred/lstm/rk"), P, 4 * P, U1 - 1, P, 4 * P, 4 * P, trans_a=True, nb1=B,
                   sA=(U1 * P, 0), sB=(U1 * 4 * P, 0), sD=(0, 0), accumulate=True)
        demb = self._dense_bwd(dz2, s["emb"], "pred/lstm/k", "pred/lstm/b")
        K.embedding_bwd(s["tokens"], demb, ps.g("pred/emb"))

    # =================================================================================== joint + loss
    def joint_fwd(self, enc, pred, B, T, U1, ctx):
        """TransducerJoint.call (base_transducer.py:280-293) -> logits [B,T,U1,V]."""
        ps, c = self.ps, self.cfg
        J, V = c.joint_dim, c.vocab_size
        e = K.matmul(enc, ps.w2d("joint/enc/w"), bias=ps.p("joint/enc/b"))
        p = K.matmul(pred, ps.w2d("joint/pred/w"), bias=ps.p("joint/pred/b"))
        h = K.joint_fwd(e.view(B, T, J), p.view(B, U1, J))
        t0 = self._tick("joint_vocab_gemm")
        logits = K.matmul(h.view(B * T * U1, J), ps.w2d("joint/vocab/w"), bias=ps.p("joint/vocab/b")).view(B, T, U1, V)
        self._tock("joint_vocab_gemm", t0, 2.0 * B * T * U1 * J * V)
        if ctx is not None:
            ctx["joint"] = dict(enc=enc, pred=pred, h=h, B=B, T=T, U1=U1)
        return logits

    def joint_bwd(self, dlogits, ctx):
        ps, c = self.ps, self.cfg
        s = ctx["joint"]
        B, T, U1 = s["B"], s["T"], s["U1"]
        J, V = c.joint_dim, c.vocab_size
        h2 = s["h"].view(B * T * U1, J)
        dh = self._dense_bwd(dlogits.view(B * T * U1, V), h2, "joint/vocab/w", "joint/vocab/b")
        de, dp = K.joint_bwd(s["h"], dh.view(B, T, U1, J))
        denc = self._dense_bwd(de.view(B * T, J), s["enc"], "joint/enc/w", "joint/enc/b")
        dpred = self._dense_bwd(dp.view(B * U1, J), s["pred"], "joint/pred/w", "joint/pred/b")
        return denc, dpred

    # =================================================================================== public API
    def __call__(self, inputs: TrainInput, training=False):
        """Transducer.call (base_transducer.py:427-435)."""
        logits, elen, _ = self._forward(inputs, training, None)
        return TrainOutput(logits=logits, logits_length=torch.tensor(elen, dtype=torch.int32))

    def _forward(self, inputs: TrainInput, training, ctx, masks=None, joint=True):
        dev = self.device
        self._drop_epoch += 1
        sig = inputs.inputs.to(dev, non_blocking=True)
        slen = [int(v) for v in inputs.inputs_length.tolist()]
        tokens = inputs.predictions.to(dev, non_blocking=True).to(torch.int32).contiguous()
        plen = inputs.predictions_length.to(dev, non_blocking=True).to(torch.int32)
        B, U1 = tokens.shape
        main = torch.cuda.current_stream()
        # Host order: the launch queue holds only ~1 ms of work, so (1) the ~1 ms of Python that draws the SpecAugment masks runs FIRST,
        # while the previous step's tail is still executing (between log-mel and the mask kernel it left the main stream idle for 0.85 ms
        # per step under the profiler's slower host; neutral in an unprofiled same-box A/B: 23.81 vs 23.85 ms), and (2) the main stream
        # gets its front end BEFORE the ~170 launches of the prediction network go to the second stream.
        if training and masks is None:
            masks = self.draw_specaugment([-(-int(n) // self.cfg.frame_step) for n in slen])
        # The front end (log-mel + SpecAugment) reads nothing a previous step wrote - no parameters, only this batch's samples - so it does
        # not have to queue behind the previous step's tail on the main stream (subsampling backward + optimizer, ~1.8 ms): it goes to the
        # prediction network's stream, idle at this point, and the main stream picks the features up (round 5; TFASR_FRONT_EARLY=0: in line).
        # Only when the CALLER says its batches are complete in HBM before train_step is called (`prefetched_inputs`, what a double-buffered
        # input pipeline - the reference's tf.data prefetch - provides and what bench.py does): a batch still being produced by earlier work
        # on the current stream would otherwise be read too early.
        if (self.prefetched_inputs and self.use_pred_stream and os.environ.get("TFASR_FRONT_EARLY", "1") != "0"
                and inputs.inputs.device.type == "cuda" and inputs.inputs.device == sig.device):
            sig.record_stream(self.pred_stream)
            with torch.cuda.stream(self.pred_stream):
                feats, flen = self.frontend(sig, slen, training, masks)
            main.wait_stream(self.pred_stream)
            feats.record_stream(main)
        else:
            feats, flen = self.frontend(sig, slen, training, masks)
        self._side_gen = None
        if self.use_pred_stream:
            self.pred_stream.wait_stream(main)
            tokens.record_stream(self.pred_stream)
            plen.record_stream(self.pred_stream)
            if self._pred_sliced():
                K.lstm_set_persist(0)
                self._side_gen = self._prediction_fwd_gen(tokens, plen, ctx)
                self._side_tick()  # embedding, input product and the first slice now; the rest between the encoder blocks
            else:
                with torch.cuda.stream(self.pred_stream):
                    pred = self.prediction_fwd(tokens, plen, ctx)
                pred.record_stream(main)
        enc, T, elen, elen_dev = self.encoder_fwd(feats, flen, training, ctx)
        if self.use_pred_stream:
            if self._side_gen is not None or getattr(self, "_side_result", None) is not None:
                self._side_drain()
                pred, self._side_result = self._side_result, None
                pred.record_stream(main)
            main.wait_stream(self.pred_stream)
        else:
            pred = self.prediction_fwd(tokens, plen, ctx)
        if not joint:
            return enc, pred, (B, T, U1), elen, elen_dev
        logits = self.joint_fwd(enc, pred, B, T, U1, ctx)
        return logits, elen, elen_dev

    def loss_and_backward(self, data: TrainData, training=True, masks=None, want_backward=True, packed=True, reduce=True):
        """BaseModel._train_step (base_model.py:149-183): forward, RnntLoss (mean over the batch, rnnt_loss.py:34) and
        the full backward into the flat gradient buffer (gradients ACCUMULATE; zero_grad() first).

        packed=True evaluates the joint network and the loss only on the valid lattice nodes (t < logit_len_b,
        u <= label_len_b): padded nodes carry exactly zero gradient in the reference (impl/rnnt.py:218-224), so skipping them
        changes no result while removing the padding's share of the largest GEMMs of the step.

        reduce=False keeps this micro-step's gradients local (train_step_ga, base_model.py:200-209: the replicas exchange
        gradients only when the accumulated gradient is applied)."""
        self.dp.set_reduce(bool(reduce))
        ctx = {} if want_backward else None
        dev = self.device
        ps, c = self.ps, self.cfg
        enc, pred, (B, T, U1), elen, elen_dev = self._forward(data.inputs, training, ctx, masks, joint=False)
        J, V = c.joint_dim, c.vocab_size
        labels = data.labels.labels.to(dev, non_blocking=True).to(torch.int32).contiguous()
        llen_host = [int(v) for v in data.labels.labels_length.tolist()]
        # BaseLoss.call: logit_length = max(logit_length, label_length)  (losses/base_loss.py:36)
        tl = [min(max(int(a), b), T) for a, b in zip(elen, llen_host)]
        ul = [min(b, U1 - 1) for b in llen_host]
        tl_dev = self._h2d(tl)
        ul_dev = self._h2d(ul)
        gkey = ("gscale", B, self.dp.world)
        if gkey not in self._consts:
            self._consts[gkey] = torch.full((B,), 1.0 / (B * self.dp.world), dtype=torch.float32, device=dev)
        gscale = self._consts[gkey]
        if not packed:
            logits = self.joint_fwd(enc, pred, B, T, U1, ctx)
            t0 = self._tick("rnnt_loss")
            costs, dlogits = K.rnnt_loss_fwd_bwd(logits, labels, ul_dev, tl_dev, grad_scale=gscale, grads=logits, want_grads=want_backward)
            self._tock("rnnt_loss", t0)
            if not want_backward:
                return costs
            denc, dpred = self.joint_bwd(dlogits, ctx)
        else:
            off = np.zeros(B + 1, np.int64)
            off[1:] = np.cumsum([t * (u + 1) for t, u in zip(tl, ul)])
            total = int(off[-1])
            off_dev = self._h2d(off, torch.int64)
            e = K.matmul(enc, ps.w2d("joint/enc/w"), bias=ps.p("joint/enc/b"))
            p = K.matmul(pred, ps.w2d("joint/pred/w"), bias=ps.p("joint/pred/b"))
            h = K.joint_fwd_packed(e.view(B, T, J), p.view(B, U1, J), off_dev, ul_dev, total)
            # The vocabulary projection's epilogue also emits the log-softmax statistics of every lattice row (max / sum-exp per
            # 64-column slice, blank and label logits) from its f32 accumulators, so the loss skips its first pass over the logits
            # (impl/rnnt.py:211 tf.nn.log_softmax + the gathers of :94-105).  bf16 fast path only; otherwise the plain route.
            stats = None
            logits = None
            if self.dtype == torch.bfloat16 and self.fuse_joint_stats:
                parts = -(-V // 128) * 2
                lse_part = torch.empty(total, parts, 2, dtype=torch.float32, device=dev)
                pick = torch.empty(total, 2, dtype=torch.float32, device=dev)
                row_label = K.rnnt_row_labels(labels, ul_dev, tl_dev, off_dev, total, T, V)
                t0 = self._tick("joint_vocab_gemm")
                if self.joint_recompute and want_backward:
                    try:
                        K.gemm(h, ps.w2d("joint/vocab/w"), None, total, V, J, J, V, V, bias=ps.p("joint/vocab/b"), lse=(lse_part, row_label, pick))
                        self._tock("joint_vocab_gemm", t0, 2.0 * total * J * V)
                        t0 = self._tick("rnnt_loss")
                        costs, coef = K.rnnt_loss_packed_coef(labels, ul_dev, tl_dev, off_dev, total, T, V, (lse_part, pick), grad_scale=gscale)
                        dlogits = torch.empty(total, V, dtype=self.dtype, device=dev)
                        K.gemm(h, ps.w2d("joint/vocab/w"), dlogits, total, V, J, J, V, V, bias=ps.p("joint/vocab/b"), rgrad=(coef, row_label))
                        # algorithmic bytes of this variant: the gradient tensor is written once (the logits never exist)
                        self._tock("rnnt_loss", t0, 1.0 * total * V * dlogits.element_size())
                        return self._joint_backward_tail(costs, dlogits, h, enc, pred, off_dev, ul_dev, tl_dev, B, T, U1, ctx)
                    except K._lib.TfasrUnsupported:
                        t0 = self._tick("joint_vocab_gemm")  # shapes outside the 256-row kernel: the materialised route below
                try:
                    logits = torch.empty(total, V, dtype=self.dtype, device=dev)
                    K.gemm(h, ps.w2d("joint/vocab/w"), logits, total, V, J, J, V, V, bias=ps.p("joint/vocab/b"), lse=(lse_part, row_label, pick))
                    stats = (lse_part, pick)
                    self._tock("joint_vocab_gemm", t0, 2.0 * total * J * V)
                except K._lib.TfasrUnsupported:
                    logits = None
                    if self.timers is not None:  # (keep the section timers paired: ADVICE r02)
                        self._tock("joint_vocab_gemm", t0, 0.0)
            if logits is None:
                t0 = self._tick("joint_vocab_gemm")
                logits = K.matmul(h, ps.w2d("joint/vocab/w"), bias=ps.p("joint/vocab/b"))  # [total, V]
                self._tock("joint_vocab_gemm", t0, 2.0 * total * J * V)
            t0 = self._tick("rnnt_loss")
            costs, dlogits = K.rnnt_loss_packed(logits, labels, ul_dev, tl_dev, off_dev, total, T, grad_scale=gscale, grads=logits,
                                                want_grads=want_backward, stats=stats)
            self._tock("rnnt_loss", t0, 2.0 * total * V * logits.element_size())
            if not want_backward:
                return costs
            return self._joint_backward_tail(costs, dlogits, h, enc, pred, off_dev, ul_dev, tl_dev, B, T, U1, ctx)
        return self._backward_from_joint(costs, denc, dpred, ctx)

    def _joint_backward_tail(self, costs, dlogits, h, enc, pred, off_dev, ul_dev, tl_dev, B, T, U1, ctx):
        """packed lattice: gradient of the lattice logits -> gradients of the joint network's inputs (+ its weight gradients)"""
        J = self.cfg.joint_dim
        ps = self.ps
        # tanh' folded into the data gradient's epilogue (dact = TANH_OUT: times 1 - h^2): the segment sums read one tensor, not two
        if self.joint_wgrad_aux and self.aux_stream is not None and isinstance(self.dp, SingleProcess) and self.dtype == torch.bfloat16:
            # one GPU: the vocabulary projection's weight gradient (nothing waits for it before the optimizer) on the auxiliary stream,
            # beside its data gradient and the start of the backward chain
            main = torch.cuda.current_stream()
            self.aux_stream.wait_stream(main)
            W = ps.w2d("joint/vocab/w")
            din, dout = W.shape
            rows = dlogits.shape[0]
            for t in (dlogits, h):
                t.record_stream(self.aux_stream)
            with torch.cuda.stream(self.aux_stream):
                K.gemm(h, dlogits, ps.g2d("joint/vocab/w"), din, dout, rows, h.stride(0), dlogits.stride(0), dout, trans_a=True, accumulate=True,
                       split_k=_split_k(din, dout, rows), colsum=ps.g("joint/vocab/b"))
            self._aux_pending = True
            dh = K.matmul(dlogits, W, trans_b=True, dact_z=h, dact=ACT_TANH_OUT)
        else:
            dh = self._dense_bwd(dlogits, h, "joint/vocab/w", "joint/vocab/b", dact_z=h, dact=ACT_TANH_OUT)
        de, dp = K.joint_bwd_packed(None, dh, off_dev, ul_dev, tl_dev, B, T, U1)
        denc = self._dense_bwd(de.view(B * T, J), enc, "joint/enc/w", "joint/enc/b")
        dpred = self._dense_bwd(dp.view(B * U1, J), pred, "joint/pred/w", "joint/pred/b")
        return self._backward_from_joint(costs, denc, dpred, ctx)

    def _backward_from_joint(self, costs, denc, dpred, ctx):
        main = torch.cuda.current_stream()
        self.dp.grads_ready(self.ps.offsets["joint/enc/w"], self.ps.n_reg)
        self._side_gen = None
        if self.use_pred_stream:
            self.pred_stream.wait_stream(main)
            dpred.record_stream(self.pred_stream)
            if self._pred_sliced():
                K.lstm_set_persist(0)
                self._side_gen = self._prediction_bwd_gen(dpred, ctx)
                self._side_tick()
            else:
                with torch.cuda.stream(self.pred_stream):
                    self.prediction_bwd(dpred, ctx)
        else:
            self.prediction_bwd(dpred, ctx)
        self.encoder_bwd(denc, ctx)
        if self.use_pred_stream:
            self._side_drain()
            main.wait_stream(self.pred_stream)
        if getattr(self, "_aux_pending", False):
            main.wait_stream(self.aux_stream)
            self._aux_pending = False
        self.dp.finish_grads()
        return costs

    # =================================================================================== greedy inference
    def get_initial_decoder_states(self, batch_size=1):
        """TransducerPrediction.get_initial_state (base_transducer.py:109-121): zeros [B, num_rnns=1, 2 (h,c), P]."""
        return torch.zeros(batch_size, 1, 2, self.cfg.rnn_units, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def align(self, data: TrainData, precision=None):
        """Forced alignment of data.labels to the audio: the best path through the lattice the loss sums over (csrc/align.hip) and the
        encoder frame at which it emits each label -> AlignOutput.  Inference mode; `precision` as in encode.  On a tie a
        label is emitted as late as possible.  Unlike the loss, the number of frames is NOT raised to the label length."""
        if (precision or self.decode_precision) == "f32" and self.dtype != torch.float32:
            return self.inference_twin().align(data, "f32")
        enc, elen = self.encode(data.inputs.inputs, data.inputs.inputs_length, "f32" if self.dtype == torch.float32 else "bf16")
        return self.align_encoded(enc, elen, data.inputs.predictions, data.labels.labels, data.labels.labels_length)

    @torch.no_grad()
    def align_encoded(self, enc, elen, predictions, labels, labels_length):
        """align() on encoder output enc [B, T', dmodel] (this model's storage type) with lengths elen: prediction network over the
        blank-prepended labels `predictions` [B, U+1], the joint network on the valid lattice nodes only, then the walk.  A bf16 model
        takes the log-probabilities from the vocabulary product's statistics epilogue (where its 256-row kernel applies the logits never
        exist); f32, or a shape that epilogue does not hold, walks materialised logits: the choices loss_and_backward makes."""
        ps, c, dev = self.ps, self.cfg, self.device
        B, T, d = enc.shape
        J, V = c.joint_dim, c.vocab_size
        tokens = predictions.to(dev).to(torch.int32).contiguous()
        no_labels = tokens.shape[1] == 1  # nothing to align anywhere: one padding column keeps the label arrays non-empty
        if no_labels:
            tokens = torch.cat([tokens, torch.full((B, 1), self.blank, dtype=torch.int32, device=dev)], 1)
        U1 = tokens.shape[1]
        lab = labels.to(dev).to(torch.int32)
        if lab.shape[1] != U1 - 1:  # labels padded to another width than the predictions
            fit = torch.zeros(B, U1 - 1, dtype=torch.int32, device=dev)
            w = min(U1 - 1, lab.shape[1])
            fit[:, :w] = lab[:, :w]
            lab = fit
        lab = lab.contiguous()
        tl = [min(max(int(v), 0), T) for v in elen]
        ul = [min(max(int(v), 0), U1 - 1) for v in labels_length.tolist()]
        tl_dev, ul_dev = self._h2d(tl), self._h2d(ul)
        plen = self._h2d([u + 1 for u in ul])
        enc2 = enc.reshape(B * T, d)
        if enc2.dtype != self.dtype or not enc2.is_contiguous():
            enc2 = K.cast(enc2.contiguous(), torch.empty(B * T, d, dtype=self.dtype, device=dev))
        pred = self.prediction_fwd(tokens, plen, None)
        off = np.zeros(B + 1, np.int64)
        off[1:] = np.cumsum([t * (u + 1) for t, u in zip(tl, ul)])
        total = int(off[-1])
        if total == 0:  # no utterance has a frame
            return AlignOutput(torch.full((B, U1 - 1), -1, dtype=torch.int32, device=dev), None, torch.zeros(B, U1 - 1, device=dev),
                               torch.full((B,), float("-inf"), device=dev), self.seconds_per_frame)
        off_dev = self._h2d(off, torch.int64)
        e = K.matmul(enc2, ps.w2d("joint/enc/w"), bias=ps.p("joint/enc/b"))
        p = K.matmul(pred, ps.w2d("joint/pred/w"), bias=ps.p("joint/pred/b"))
        h = K.joint_fwd_packed(e.view(B, T, J), p.view(B, U1, J), off_dev, ul_dev, total)
        out = None
        if self.dtype == torch.bfloat16 and self.fuse_joint_stats:
            parts = -(-V // 128) * 2
            lse_part = torch.empty(total, parts, 2, dtype=torch.float32, device=dev)
            pick = torch.empty(total, 2, dtype=torch.float32, device=dev)
            row_label = K.rnnt_row_labels(lab, ul_dev, tl_dev, off_dev, total, T, V)
            # statistics only (the 256-row kernel), else statistics beside materialised logits (the 128-row kernel: the walk still skips its
            # pass over them), else the plain route below: the order loss_and_backward tries them in
            for materialise in (False, True):
                try:
                    logits = torch.empty(total, V, dtype=self.dtype, device=dev) if materialise else None
                    K.gemm(h, ps.w2d("joint/vocab/w"), logits, total, V, J, J, V, V, bias=ps.p("joint/vocab/b"), lse=(lse_part, row_label, pick))
                    out = K.rnnt_align_stats((lse_part, pick), lab, ul_dev, tl_dev, T, V, cell_off=off_dev, blank=self.blank)
                    break
                except K._lib.TfasrUnsupported:
                    out = None
        if out is None:
            logits = K.matmul(h, ps.w2d("joint/vocab/w"), bias=ps.p("joint/vocab/b"))  # [total, V]
            out = K.rnnt_align(logits, lab, ul_dev, tl_dev, T=T, cell_off=off_dev, blank=self.blank)
        frames, label_lp, score = out
        if no_labels:
            frames, label_lp = frames[:, :0], label_lp[:, :0]
        return AlignOutput(frames, None, label_lp, score, self.seconds_per_frame)

    @torch.no_grad()
    def recognize(self, inputs: PredictInput, max_tokens_per_frame=3, check_every=16, precision=None):
        """Transducer.recognize (base_transducer.py:474-494): batch size 1 -> recognize_single (<=3 symbols per frame),
        otherwise recognize_batch — the two variants are NOT equivalent in the reference and both are reproduced."""
        enc, elen = self.encode(inputs.inputs, inputs.inputs_length, precision)
        out = self.recognize_encoded(enc, elen, inputs.previous_tokens, inputs.previous_decoder_states, max_tokens_per_frame,
                                     check_every)
        if inputs.previous_encoder_states is not None:  # a streaming session's encoder state (streaming.StreamState.export) rides along
            out = out._replace(next_encoder_states=inputs.previous_encoder_states)
        return out

    def recognize_beam(self, inputs: PredictInput, beam_width=10, device_search=False, precision=None, **kw):
        """The reference's recognize_beam falls back to greedy (base_transducer.py:841-842), and so does this one by default.
        device_search=True runs the modified beam search on the device (csrc/rnnt_beam.hip: at most one symbol per frame, equal label
        sequences merged) and returns its best path: tokens [B, T'] blank padded, next_tokens [B, 1], next_decoder_states [B, 1, 2, P]."""
        if not device_search:
            return self.recognize(inputs, precision=precision, **kw)
        enc, elen = self.encode(inputs.inputs, inputs.inputs_length, precision)
        tokens, _, _, next_tok, states = self.recognize_beam_encoded(enc, elen, beam_width, 1, inputs.previous_tokens,
                                                                     inputs.previous_decoder_states)
        return PredictOutput(tokens=tokens[:, 0], next_tokens=next_tok[:, :1], next_encoder_states=None, next_decoder_states=states[:, 0])

    def recognize_nbest(self, inputs: PredictInput, beam_width=10, top_paths=4, precision=None):
        """n-best list of the device beam search: (tokens [B, NP, T'] blank padded, lengths [B, NP], scores [B, NP]), best first; paths
        past the last live hypothesis are empty with score -inf (the shapes of ConformerCTC.recognize_nbest)."""
        enc, elen = self.encode(inputs.inputs, inputs.inputs_length, precision)
        tokens, lengths, scores, _, _ = self.recognize_beam_encoded(enc, elen, beam_width, top_paths, inputs.previous_tokens,
                                                                    inputs.previous_decoder_states)
        return tokens, lengths, scores

    @torch.no_grad()
    def recognize_nbest_detailed(self, inputs: PredictInput, beam_width=10, top_paths=4, precision=None):
        """recognize_nbest that also says when each token of each hypothesis was spoken and how sure the model was -> NBestOutput (ends
        None).  ONE encoder pass: recognize_beam_encoded on its output, then align_encoded on the same rows repeated once per path, with
        the hypotheses as labels and their blank-prepended form as predictions - on the model align() would use (a bf16 model's f32
        twin by default, whose encoder output `encode` already returned).  frames / log_probs are align_encoded's; entropies: the joint
        activation of each label's emitting node (frames[u], u) is gathered, projected with the vocabulary weights (one product of
        [B * P * U, joint_dim] rows) and reduced by tfasr_row_lse_entropy; for this the encoder projection and the prediction network of
        the hypotheses run a second time, beside align_encoded's own.  path_scores: the alignment's score, -inf for a path past the last
        live hypothesis.  The alignment starts from the blank and the zero state: other previous tokens or states are refused."""
        if inputs.previous_tokens is not None or inputs.previous_decoder_states is not None:
            raise ValueError("recognize_nbest_detailed aligns from the blank and the zero prediction state: previous_tokens / "
                             "previous_decoder_states must be None")
        enc, elen = self.encode(inputs.inputs, inputs.inputs_length, precision)
        toks, lengths, scores, _, _ = self.recognize_beam_encoded(enc, elen, beam_width, top_paths)
        al = self.inference_twin() if (precision or self.decode_precision) == "f32" else self  # align()'s rule; enc has al's type
        dev, c = self.device, self.cfg
        B, NP, W = toks.shape
        T, J, V = enc.shape[1], c.joint_dim, c.vocab_size
        R = B * NP
        n = lengths.reshape(R).clamp(min=0)
        U = int(n.max().item())
        frames = torch.full((B, NP, W), -1, dtype=torch.int32, device=dev)
        logp = torch.zeros(B, NP, W, dtype=torch.float32, device=dev)
        ent = torch.zeros(B, NP, W, dtype=torch.float32, device=dev)
        lab = toks.reshape(R, W)[:, :U].contiguous()
        pred_tok = torch.cat([torch.full((R, 1), self.blank, dtype=torch.int32, device=dev), lab], 1)
        elen_r = [int(v) for v in elen for _ in range(NP)]
        a = al.align_encoded(enc.repeat_interleave(NP, 0), elen_r, pred_tok, lab, n.cpu())
        dead = scores == float("-inf")
        path = torch.where(dead, scores, a.scores.view(B, NP))
        if U > 0:
            fr = torch.where(dead.view(R, 1), torch.full_like(a.frames, -1), a.frames)
            lp = torch.where(fr >= 0, a.label_log_probs, torch.zeros_like(a.label_log_probs))
            # the emitting node of label u is (frames[u], u): encoder row b * T + frames[u], prediction row r * (U + 1) + u
            # (all B * T encoder rows are projected: the B * P * U gathered rows are not fewer in general, and repeat rows)
            e = K.matmul(enc.reshape(B * T, enc.shape[2]).contiguous(), al.ps.w2d("joint/enc/w"), bias=al.ps.p("joint/enc/b"))
            p = K.matmul(al.prediction_fwd(pred_tok.contiguous(), (n + 1).to(torch.int32), None), al.ps.w2d("joint/pred/w"),
                         bias=al.ps.p("joint/pred/b"))
            rows = torch.arange(R, device=dev).view(R, 1)
            ei = ((rows // NP) * T + fr.clamp(min=0)).reshape(-1)
            pi = (rows * (U + 1) + torch.arange(U, device=dev).view(1, U)).reshape(-1)
            h = K.joint_fwd(e.index_select(0, ei).view(R * U, 1, J), p.index_select(0, pi).view(R * U, 1, J)).view(R * U, J)
            logits = K.matmul(h, al.ps.w2d("joint/vocab/w"), bias=al.ps.p("joint/vocab/b"))
            h_ent = K.row_lse_entropy(logits.view(R * U, V))[1].view(R, U)
            frames[:, :, :U] = fr.view(B, NP, U)
            logp[:, :, :U] = lp.view(B, NP, U)
            ent[:, :, :U] = torch.where(fr >= 0, h_ent, torch.zeros_like(h_ent)).view(B, NP, U)
        return NBestOutput((toks, lengths, scores), toks, lengths, frames, None, logp, ent, path, self.seconds_per_frame, V)

    @torch.no_grad()
    def recognize_beam_encoded(self, enc, elen, beam_width=10, top_paths=1, previous_tokens=None, previous_decoder_states=None):
        """The device beam search on encoder output enc [B, T', dmodel] with lengths elen: (tokens [B, NP, T'], lengths [B, NP], scores
        [B, NP] f32, next_tokens [B, NP], next_decoder_states [B, NP, 1, 2, P]).  Path p continues from next_tokens[:, p:p+1] and
        next_decoder_states[:, p] (the greedy search's convention: the path's last label, or the initial token, and the prediction
        state before it is fed).  f32 on the f32 master weights whatever the model's storage type, as recognize_encoded."""
        ps, c, dev = self.ps, self.cfg, self.device
        B, T, d = enc.shape
        P, J = c.rnn_units, c.joint_dim
        f32 = torch.float32
        lens = [min(max(int(v), 0), T) for v in elen]
        Tm = max(max(lens), 1)  # frames past every utterance are never searched
        enc32 = enc[:, :Tm].reshape(B * Tm, d)
        if enc32.dtype != f32 or not enc32.is_contiguous():
            enc32 = K.cast(enc32.contiguous(), torch.empty(B * Tm, d, dtype=f32, device=dev))
        encj = K.matmul(enc32, ps.p2d("joint/enc/w"), bias=ps.p("joint/enc/b")).view(B, Tm, J)
        init_tok = None if previous_tokens is None else previous_tokens.to(dev).to(torch.int32).reshape(B).contiguous()
        init_h = init_c = None
        if previous_decoder_states is not None:
            st = previous_decoder_states.to(dev)
            init_h, init_c = st[:, 0, 0].float().contiguous(), st[:, 0, 1].float().contiguous()
        lng, lnb = (ps.p("pred/ln/g"), ps.p("pred/ln/b")) if c.prediction_layer_norm else (None, None)
        Wk, Wrk, Wjp, Wv = ps.p2d("pred/lstm/k"), ps.p2d("pred/lstm/rk"), ps.p2d("joint/pred/w"), ps.p2d("joint/vocab/w")
        toks, lengths, scores, next_tok, next_h, next_c = K.rnnt_beam_search(
            ps.p("pred/emb"), Wk, Wrk, ps.p("pred/lstm/b"), lng, lnb, Wjp, ps.p("joint/pred/b"), Wv, ps.p("joint/vocab/b"), encj,
            torch.tensor(lens, dtype=torch.int32), beam_width, top_paths, self.blank, init_tok, init_h, init_c)
        if Tm < T:
            full = torch.full((B, toks.shape[1], T), self.blank, dtype=torch.int32, device=dev)
            full[:, :, :Tm] = toks
            toks = full
        states = torch.stack([next_h, next_c], dim=2).unsqueeze(2)  # [B, NP, 1, 2, P]
        return toks, lengths, scores, next_tok, states

    @torch.no_grad()
    def recognize_encoded(self, enc, elen, previous_tokens=None, previous_decoder_states=None, max_tokens_per_frame=3,
                          check_every=16):
        return self._greedy_search(enc, elen, previous_tokens, previous_decoder_states, max_tokens_per_frame, check_every, False)[0]

    @torch.no_grad()
    def recognize_detailed(self, inputs: PredictInput, max_tokens_per_frame=3, check_every=16, precision=None):
        """recognize that also says when each token was spoken and how sure the model was -> RecognizeOutput (schemas.token_times,
        token_confidences, word_details read it).  Same search, same tokens: the bookkeeping kernel keeps, next to every symbol it writes,
        the frame, the log-probability and the entropy of the decision (tfasr_decode_update_detail) - no second pass over the encoder."""
        enc, elen = self.encode(inputs.inputs, inputs.inputs_length, precision)
        out = self.recognize_encoded_detailed(enc, elen, inputs.previous_tokens, inputs.previous_decoder_states, max_tokens_per_frame,
                                              check_every)
        if inputs.previous_encoder_states is not None:
            out = out._replace(predict=out.predict._replace(next_encoder_states=inputs.previous_encoder_states))
        return out

    @torch.no_grad()
    def recognize_encoded_detailed(self, enc, elen, previous_tokens=None, previous_decoder_states=None, max_tokens_per_frame=3,
                                   check_every=16):
        """recognize_encoded -> RecognizeOutput: frames / log_probs / entropies [B, W] column-aligned with predict.tokens (a batch: symbols
        from column 2; -1 / 0 where no symbol sits), ends None, scores [B] = the sum of the emitted tokens' log-probabilities."""
        out, (frames, logp, ent) = self._greedy_search(enc, elen, previous_tokens, previous_decoder_states, max_tokens_per_frame,
                                                       check_every, True)
        scores = torch.where(frames >= 0, logp, torch.zeros_like(logp)).sum(1)
        return RecognizeOutput(out, frames, None, logp, ent, scores, self.seconds_per_frame, self.cfg.vocab_size)

    def _greedy_search(self, enc, elen, previous_tokens, previous_decoder_states, max_tokens_per_frame, check_every, detail):
        """The greedy search of recognize_encoded -> (PredictOutput, None), or with `detail` (PredictOutput, (tok_frames, tok_logp,
        tok_entropy)): the same launches with the detail variant of the bookkeeping kernel."""
        ps, c, dev = self.ps, self.cfg, self.device
        B, T, d = enc.shape
        E, P, J, V = c.embed_dim, c.rnn_units, c.joint_dim, c.vocab_size
        mode = 1 if B == 1 else 0
        # The search arithmetic (embedding, LSTM cell, LayerNorm, joint, vocabulary projection, log-softmax, arg-max) runs in
        # f32 on the f32 master weights whatever the model's storage type: the GEMMs of one step are [B, <=640] x [640, <=2560]
        # (launch-bound, not MFMA-bound), and every token decision then carries the reference's f32 arithmetic
        # (base_transducer.py:437-464) - a bf16 model's tokens are bit-exact against the reference search applied to ITS
        # encoder output (tests/test_parity_baseline_gpu.py).
        f32 = torch.float32
        nframes = torch.tensor([int(v) for v in elen], dtype=torch.int32).to(dev)
        enc32 = enc.reshape(B * T, d)
        if enc32.dtype != f32:
            enc32 = K.cast(enc32.contiguous(), torch.empty(B * T, d, dtype=f32, device=dev))
        encj = K.matmul(enc32, ps.p2d("joint/enc/w"), bias=ps.p("joint/enc/b")).view(B, T, J)
        max_tokens = int(elen[0]) * max_tokens_per_frame if mode == 1 else 2 * T + 1
        tokens = torch.full((B, max(max_tokens, 1)), self.blank, dtype=torch.int32, device=dev)
        det = ()  # detail buffers, shaped like `tokens`
        if detail:
            det = (torch.full_like(tokens, -1), torch.zeros(tokens.shape, dtype=f32, device=dev), torch.zeros(tokens.shape, dtype=f32, device=dev))
        steps, update = (K.decode_steps_detail, K.decode_update_detail) if detail else (K.decode_steps, K.decode_update)
        frame_idx = torch.zeros(B, dtype=torch.int32, device=dev)
        tok_idx = torch.full((B,), -1 if mode == 1 else 1, dtype=torch.int32, device=dev)
        prev_tok = (torch.full((B,), self.blank, dtype=torch.int32, device=dev) if previous_tokens is None
                    else previous_tokens.to(dev).to(torch.int32).reshape(B).clone())  # (updated in place by the search: never the caller's tensor)
        if previous_decoder_states is None:
            h = torch.zeros(B, P, dtype=f32, device=dev)
            cst = torch.zeros(B, P, dtype=f32, device=dev)
        else:
            st = previous_decoder_states.to(dev)
            h = st[:, 0, 0].float().clone()
            cst = st[:, 0, 1].float().clone()
        per_frame = torch.zeros(max(int(elen[0]), 1), dtype=torch.int32, device=dev) if mode == 1 else None
        active = torch.ones(1, dtype=torch.int32, device=dev)
        ecur = torch.empty(B, J, dtype=f32, device=dev)
        xg = torch.empty(B, 4 * P, dtype=f32, device=dev)
        hr = torch.empty(B, 4 * P, dtype=f32, device=dev)
        h_new = torch.empty(B, P, dtype=f32, device=dev)
        c_new = torch.empty(B, P, dtype=f32, device=dev)
        pj = torch.empty(B, J, dtype=f32, device=dev)
        logits = torch.empty(B, V, dtype=f32, device=dev)
        Wk, Wrk, Wjp, Wv = ps.p2d("pred/lstm/k"), ps.p2d("pred/lstm/rk"), ps.p2d("joint/pred/w"), ps.p2d("joint/vocab/w")
        # every useful iteration advances a frame or appends a token; the reference's while_loop is unbounded and can
        # spin forever once a sample saturates its token buffer — cap the trip count instead
        max_iters = T + max_tokens + 2
        it = 0
        zbuf = torch.empty(B, J, dtype=f32, device=dev)
        lng, lnb = (ps.p("pred/ln/g"), ps.p("pred/ln/b")) if c.prediction_layer_norm else (None, None)
        fused = B <= 64 and self.decode_fused
        packed = K.decode_pack(ps.p("pred/emb"), Wk, Wrk, Wjp, Wv) if fused else None  # tile order of the MFMA step kernels
        # Iterations queued per host check (fused route).  A row leaves the loop only after it has consumed its frames, one per blank, so
        # max_b(frames left) iterations are certain to be needed: that many are queued without looking (the first batch is ~T' long), then
        # the counters are read back ONCE per batch (one device -> host sync) - 4-5 syncs per search instead of one per 64 iterations; the
        # no-op tail of the last batch is at most `check_every` iterations.
        need = int(elen[0]) - 1 if mode == 1 else max(int(v) for v in elen) - 1
        while it < max_iters:
            n = min(max(need, check_every) if fused else check_every, max_iters - it)
            if fused:
                # `n` iterations = 3 skinny-product launches + the bookkeeping kernel each (csrc/decode_step.hip), queued by one host call
                fused = steps(ps.p("pred/emb"), Wk, Wrk, ps.p("pred/lstm/b"), lng, lnb, Wjp, ps.p("joint/pred/b"), Wv,
                              ps.p("joint/vocab/b"), encj, nframes, frame_idx, tok_idx, prev_tok, h, cst, active, h_new, c_new, zbuf,
                              logits, tokens, per_frame, *det, max_tokens, self.blank, mode, max_tokens_per_frame, n, packed=packed)
                if fused:
                    it += n
                    left = (nframes - 1 - frame_idx).clamp_(min=0).max()
                    act_h, need = (int(v) for v in torch.stack([active[0], left]).tolist())  # (one sync)
                    if act_h == 0:
                        break
                    continue
            for _ in range(n):
                K.decode_prepare(encj, nframes, frame_idx, tok_idx, active, ecur, max_tokens, mode)
                emb = K.embedding_fwd(prev_tok, ps.p("pred/emb"), f32)
                K.matmul(emb, Wk, bias=ps.p("pred/lstm/b"), out=xg)
                K.gemm(h, Wrk, hr, B, 4 * P, P, P, 4 * P, 4 * P)
                K.lstm_step_fwd(xg, hr, h, cst, None, 0, None, c_new, h_new, None, B, P)
                if c.prediction_layer_norm:
                    y, _, _ = K.layernorm_fwd(h_new, ps.p("pred/ln/g"), ps.p("pred/ln/b"), save_stats=False)
                else:  # prediction_layer_norm: False (contextnet/small.yml.j2), as prediction_fwd
                    y = h_new
                K.matmul(y, Wjp, bias=ps.p("joint/pred/b"), out=pj)
                z = K.joint_fwd(ecur.view(B, 1, J), pj.view(B, 1, J))
                K.matmul(z.view(B, J), Wv, bias=ps.p("joint/vocab/b"), out=logits)
                update(logits, active, nframes, frame_idx, prev_tok, tok_idx, tokens, per_frame, h_new, c_new, h, cst, *det,
                       max_tokens, self.blank, mode, max_tokens_per_frame)
                it += 1
            if int(active.item()) == 0:
                break
        self.last_search_iterations = it  # (queued iterations incl. the no-op tail of the last batch; bench.py reports it)
        states = torch.stack([h, cst], dim=1).unsqueeze(1)  # [B, 1, 2, P]
        out = PredictOutput(tokens=tokens[:, :max_tokens], next_tokens=prev_tok.view(B, 1), next_encoder_states=None,
                            next_decoder_states=states)
        return out, (tuple(t[:, :max_tokens] for t in det) if detail else None)
