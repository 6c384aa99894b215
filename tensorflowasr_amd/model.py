"""What every model of the package is, whatever its encoder and head: AsrModel (see its docstring for the seam between the three layers).

Mirrors the part of the reference's model surface that does not depend on the architecture:
    FeatureExtraction.call, SpecAugment                         (feature_extraction.py:255-303, specaugment.py, augmentation.py)
    BaseModel.train_step / _train_step / _apply_gradients       (models/base_model.py:149-198)
but is NOT a Keras graph: every module has a hand-written backward that reuses the forward's saved tensors, and a step is a fixed sequence
of C-ABI kernel launches.  PyTorch only owns device memory and streams here.  There is no CPU / eager fallback.
"""
import math
import os

import numpy as np
import torch

from . import kernels as K
from .base_model import BaseModel
from .kernels import ACT_NONE
from .params import ParamStore
from .schemas import TrainData


class SingleProcess:
    """Collective hooks for one GPU (tensorflowasr_amd.dp.DataParallel implements them over RCCL)."""

    world = 1
    rank = 0

    def allreduce_stats_(self, t):  # sync-BN statistics (sum over replicas)
        return t

    def set_reduce(self, on):  # gradient accumulation: only the apply micro-step exchanges gradients
        pass

    def grads_ready(self, lo, hi):  # gradient slice [lo, hi) of the flat buffer is final
        pass

    def finish_grads(self):
        pass


def _split_k(M, N, Kd):
    tiles = -(-M // 128) * -(-N // 128)
    if tiles >= 512 or Kd <= 2048:
        return 1
    v = int(max(1, min(-(-1024 // tiles), Kd // 1024, 64)))
    return (v + 4) // 8 * 8 if v >= 12 else v  # whole k-slices per XCD (gemm_fast.hip split-K mapping needs split % 8 == 0)


class AsrModel(BaseModel):
    """A model = an ENCODER mixin in front of a HEAD, over this base:  class ConformerCTC(ConformerEncoderMixin, CtcModel).
    The data path is  frontend -> encoder_fwd -> head  and back  head -> encoder_bwd;  construction runs here and calls one hook per layer.

    An encoder provides
        encoder_kind                                  the cfg.encoder it is built for
        encoder_fwd(feats, flen, training, ctx)       features [B, T0, F], frame counts (host) -> ([B*T', dmodel], T', lengths host, lengths
                                                      device); with ctx (a dict) it saves there what its backward needs
        encoder_bwd(dx, ctx)                          if it trains: gradient of encoder_fwd's output -> all its parameter gradients, complete
                                                      and released to self.dp (grads_ready) when it returns
        _encoder_length(t)                            feature frames -> encoder frames (BaseModel's default is the Conformer's)
        _init_encoder()                               its state and switches, after self.ps / self.dp exist
        _param_options(cfg, dtype)                    optional: keyword arguments for its ParamStore (padded physical sizes)
        _reset_caches()                               optional, through super(): per-instance caches that depend on the storage type
        stream(...)                                   if it streams (streaming.STREAM_STATES names its state class)
    and calls self._side_tick() between its blocks, in both directions (a head may have work to queue beside it).

    A head (TransducerModel, CtcModel) provides
        head_kind                                     the cfg.head it is built for
        _init_head()                                  its state, switches and streams
        __call__, loss_and_backward                   forward / loss / backward around encoder_fwd and encoder_bwd
        recognize, recognize_detailed, recognize_beam, recognize_nbest, align, get_initial_decoder_states
        _side_tick()                                  optional: queue a slice of its own work on its own stream

    The base guarantees both
        cfg, device, dtype, ps (the ParamStore), dp (collective hooks), blank, step, _rng, _consts (per-instance constants)
        frontend / draw_specaugment, _h2d, dropout seeds (_drop), _dense_bwd, BatchNorm (_bn_fwd / _bn_bwd, _zeros_f32), _tick / _tock
        the optimiser and train_step, encode, inference_twin (same parameters in f32; caches of _reset_caches fresh, the rest shared),
        and the streaming entry points that only dispatch on the encoder's state class."""

    encoder_kind = None
    head_kind = None
    _config_error = None  # the concrete class's sentence for a config of another encoder / head

    def __init__(self, cfg, device=None, dtype=torch.bfloat16, seed=0, dp=None):
        if getattr(cfg, "encoder", "conformer") != self.encoder_kind or getattr(cfg, "head", "transducer") != self.head_kind:
            raise ValueError(self._config_error)
        if not torch.cuda.is_available():
            raise K._lib.TfasrError("ConformerTransducer needs an MI355X (HIP) device; there is no CPU fallback")
        self.cfg = cfg
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.dtype = dtype
        self.ps = ParamStore(cfg, self.device, dtype, seed, **self._param_options(cfg, dtype))
        self.dp = dp or SingleProcess()
        self.blank = cfg.blank
        self.time_reduction_factor = cfg.time_reduction_factor
        self.step = 0
        self._reset_caches()
        # SpecAugment draws and dropout masks are per replica (MirroredStrategy draws independent randomness on every
        # replica); the parameter initialisation seed above is shared by all ranks
        self._rng = np.random.default_rng([seed + 1000, int(self.dp.rank)])
        self.optimizer = dict(beta1=0.9, beta2=0.98, eps=1e-9, weight_decay=1e-6, schedule=dict(
            dmodel=cfg.dmodel, warmup_steps=10000, scale=2.0, max_lr=0.05 / math.sqrt(cfg.dmodel)))
        self.ga_steps = 1
        self.prefetched_inputs = False  # True: every batch handed to train_step is complete in HBM (see TransducerModel._forward: early front end)
        self._ga_count = 0
        self._drop_epoch = 0  # bumped once per forward pass so every step draws fresh dropout masks
        self.timers = None  # optional dict name -> list[(start_event, end_event)] filled by bench.py
        self.timer_work = {}
        self.time_sections = False  # per-module section timers (bench.py TFASR_BENCH_SECTIONS) need the per-kernel Python path
        # Greedy search: the reference's tokens come from its f32 CPU path and the north star asks for bit-exact token indices, which a
        # bf16 encoder cannot promise (near-tied arg-max decisions flip).  Inference therefore runs on the f32 master weights with the
        # exact-f32 MFMA kernels by default, whatever the training storage type ("bf16" = the training kernels, faster, not token-exact)
        self.decode_precision = os.environ.get("TFASR_DECODE_PRECISION", "f32")
        self._twin = None
        # Streams = hardware queues, and on this chip the step time depends on how many are live (with eight queues a
        # data-parallel rank ran 38 instead of 23 ms).  HIP never lets streams of DIFFERENT priority share a queue, so the three streams of the
        # step sit on three priority levels - the encoder chain on the default stream, the prediction network (hundreds of tiny launches the
        # joint network waits for) on a HIGH-priority stream, everything nothing on the chain waits for on the executor's LOW-priority stream -
        # which keeps them on separate queues whatever GPU_MAX_HW_QUEUES is and whatever streams RCCL adds.  Each is created by the layer
        # that launches on it: the head first, then the encoder.
        self._init_head()
        self._init_encoder()

    # =================================================================================== hooks of the encoder and the head (see the class docstring)
    def _param_options(self, cfg, dtype):
        return {}

    def _init_head(self):
        pass

    def _init_encoder(self):
        pass

    def _reset_caches(self):
        self._consts = {}

    def _side_tick(self):
        pass

    # =================================================================================== constants
    def _frontend_consts(self):
        if "fe" not in self._consts:
            c = self.cfg
            n = c.frame_length
            window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)).astype(np.float32)  # periodic Hann
            melw = _mel_weight_matrix(c.num_feature_bins, c.nfft // 2 + 1, c.sample_rate, c.lower_edge_hertz, c.upper_edge_hertz)
            band = np.zeros((melw.shape[1], 2), np.int32)
            for m in range(melw.shape[1]):
                nz = np.nonzero(melw[:, m])[0]
                band[m] = (nz[0], nz[-1]) if len(nz) else (0, -1)
            dev = self.device
            self._consts["fe"] = (torch.from_numpy(window).to(dev), torch.from_numpy(melw).to(dev), torch.from_numpy(band).to(dev))
        return self._consts["fe"]

    # =================================================================================== dropout bookkeeping
    def _drop(self, site, training):
        """(rate, seed) of dropout site `site` for the current step; masks are a pure function of (seed, element index), so
        the backward regenerates them instead of storing them (keras Dropout sites: conformer.py:80-87,197,358,681)."""
        p = float(self.cfg.dropout) if training else 0.0
        if p <= 0.0:
            return 0.0, 0
        return p, (self._drop_epoch_eff() * 8192 + site) & 0x7FFFFFFFFFFF

    def _drop_epoch_eff(self):
        """Mask epoch with the data-parallel rank folded into bits 40..46 of the seed (epoch * 8192 + site stays below 2^40
        for 2^27 forward passes): replicas draw different dropout masks; the native block executor forms the same seed."""
        return self._drop_epoch + ((int(self.dp.rank) & 0x7F) << 27)

    def _mask_grad(self, dy, drop):
        return K.dropout(dy, drop[0], drop[1]) if drop[0] > 0.0 else dy

    # =================================================================================== dense helpers
    def _dense_bwd(self, dy, x, wname, bname, alpha=1.0, dact_z=None, dact=ACT_NONE, need_dx=True, drop=(0.0, 0)):
        """dx = alpha * (dy @ W^T) [* dact'(z)];  gW += alpha * x^T dy;  gb += alpha * colsum(dy)."""
        ps = self.ps
        W = ps.w2d(wname)
        rows = dy.shape[0]
        din, dout = W.shape
        # weight gradient; the bias gradient (column sums of dy) rides in the same launch
        K.gemm(x, dy, ps.g2d(wname), din, dout, rows, x.stride(0), dy.stride(0), dout, trans_a=True, accumulate=True,
               split_k=_split_k(din, dout, rows), alpha=alpha, colsum=ps.g(bname) if bname is not None else None)
        if not need_dx:
            return None
        return K.matmul(dy, W, trans_b=True, alpha=alpha, dact_z=dact_z, dact=dact, drop_p=drop[0], drop_seed=drop[1])

    def _h2d(self, x, dtype=torch.int32):
        """Small host array -> device through PINNED staging: a pageable hipMemcpyAsync makes the host wait until the stream
        has drained up to the copy, which stops the host from queueing kernels ahead of the GPU several times per step."""
        t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
        t = t.to(dtype)
        if t.device.type == "cpu":
            if self.device.type == "cuda":
                t = t.pin_memory()
            t = t.to(self.device, non_blocking=True)
        return t

    # =================================================================================== frontend
    def frontend(self, signals, signals_length, training=False, masks=None):
        """FeatureExtraction.call (feature_extraction.py:255-303) -> features [B,T0,F] (compute dtype), feature lengths (host)."""
        c = self.cfg
        window, melw, band = self._frontend_consts()
        feats = K.logmel(signals, window, melw, band, c.frame_step, c.nfft, c.preemphasis, c.epsilon, self.dtype)
        flen = [-(-int(n) // c.frame_step) for n in signals_length]
        if training:
            if masks is None:
                masks = self.draw_specaugment(flen)
            fm, tm = masks
            if fm is not None or tm is not None:
                K.specaugment(feats, None if fm is None else self._h2d(fm), None if tm is None else self._h2d(tm), 0.0)
        return feats, flen

    def draw_specaugment(self, flen):
        """Random draws of FreqMasking/TimeMasking.augment (specaugment.py:72-77,122-131; freq before time:
        augmentation.py:95; TimeMasking ignores mask_factor)."""
        c = self.cfg
        fcfg, tcfg = c.freq_masking, c.time_masking
        B = len(flen)
        rng = self._rng
        nf = fcfg.get("num_masks", 0) if fcfg else 0
        nt = tcfg.get("num_masks", 0) if tcfg else 0
        fm = np.zeros((B, nf, 2), np.int32) if nf > 0 else None
        tm = np.zeros((B, nt, 2), np.int32) if nt > 0 else None
        nb = c.num_feature_bins
        # the reference's consumption order: utterance by utterance (tf.map_fn, augmentation.py:78-90), frequency masks before time
        # masks, and per mask (prob, width, start) are drawn unconditionally and multiplied by do_apply afterwards
        # (hot host loop, ~1 000 generator calls per batch: lookups hoisted; rng.random() is uniform(0, 1) - same stream, same values)
        rnd, rint = rng.random, rng.integers
        fprob = fcfg.get("prob", 1.0) if fcfg else 1.0
        fmax = max(1, int(fcfg["mask_factor"])) if nf > 0 else 1
        tprob = tcfg.get("prob", 1.0) if tcfg else 1.0
        tup = np.float32(tcfg.get("p_upperbound", 1.0)) if tcfg else np.float32(1.0)
        for b in range(B):
            ln = int(flen[b])
            for k in range(nf):
                do = 1 if rnd() <= fprob else 0
                f = do * min(int(rint(0, fmax)), nb)
                fm[b, k] = (do * int(rint(0, max(1, nb - f))), f)
            if nt > 0:
                Tb = max(1, int(math.floor(np.float32(ln) * tup)))
            for k in range(nt):
                do = 1 if rnd() <= tprob else 0
                # tf.random.uniform(maxval=0) is an InvalidArgumentError in the reference (fewer than 20 frames at 0.05):
                # a zero-width mask here
                t = do * min(int(rint(0, Tb)), ln)
                tm[b, k] = (do * int(rint(0, max(1, ln - t))), t)
        return (None if fm is None else torch.from_numpy(fm)), (None if tm is None else torch.from_numpy(tm))

    # =================================================================================== batch norm
    def _zeros_f32(self, n):
        """n zeroed f32 accumulators for one launch (BN sums): slices of an arena cleared by ONE fill per ~1 MB instead of one fill
        launch per use (the ContextNet step had 300 of them).  An exhausted arena is replaced, never re-cleared, so slices that are
        still referenced stay valid."""
        n = (n + 63) // 64 * 64
        size = max(1 << 18, n)
        arena, cur = self._consts.get("zero_arena", (None, 0))
        if arena is None or cur + n > arena.numel():
            arena, cur = torch.zeros(size, dtype=torch.float32, device=self.device), 0
        self._consts["zero_arena"] = (arena, cur + n)
        return arena[cur:cur + n]

    def _bn_fwd(self, x2d, name, training, act, rows=None, y=None):
        """rows: number of REAL rows when x2d carries exactly-zero padding rows (haloed layouts): zeros change neither sum."""
        ps = self.ps
        C = x2d.shape[1]
        fin = torch.empty(4 * C, dtype=torch.float32, device=self.device)
        if training:
            stats = self._zeros_f32(2 * C + 1)[:2 * C + 1]
            K.bn_stats(x2d, stats)
            count = (x2d.shape[0] if rows is None else rows) * self.dp.world
            self.dp.allreduce_stats_(stats[:2 * C])
        else:
            stats, count = None, x2d.shape[0]
        # statistics -> coefficients (+ moving statistics) -> normalise + activation in ONE launch where the row kernel applies
        got = K.bn_finalize_apply_fwd(x2d, stats, count if training else 1, ps.p(name + "/g"), ps.p(name + "/b"), fin, ps.state[name + "/mm"],
                                      ps.state[name + "/mv"], act, y=y, training=training)
        if got is None:
            K.bn_finalize(stats, count if training else 1, ps.p(name + "/g"), ps.p(name + "/b"), fin, ps.state[name + "/mm"], ps.state[name + "/mv"],
                          0.99, 1e-3, training)
            got = K.bn_apply_fwd(x2d, fin, act, y=y)
        return got, (fin, count)

    def _bn_bwd(self, x2d, dy2d, name, saved, act, dx=None):
        fin, count = saved
        ps = self.ps
        C = x2d.shape[1]
        bstats = self._zeros_f32(2 * C)[:2 * C]
        K.bn_bwd_stats(x2d, dy2d, fin, bstats, act)
        self.dp.allreduce_stats_(bstats)
        # bstats = (sum dz, sum dz*xhat) over the GLOBAL batch = the beta / gamma gradients; the flat-gradient all-reduce sums over ranks again
        return K.bn_apply_bwd(x2d, dy2d, fin, bstats, count, act, dx=dx, dgamma=ps.g(name + "/g"), dbeta=ps.g(name + "/b"), grad_scale=1.0 / self.dp.world)

    def zero_grad(self):
        self.ps.grad.zero_()

    def learning_rate(self, step):
        s = self.optimizer["schedule"]
        if isinstance(s, (int, float)):
            return float(s)
        from .configs import transformer_schedule

        return transformer_schedule(step, **s)

    def apply_gradients(self, grad_scale=1.0):
        """BaseModel._apply_gradients -> keras Adam (base_model.py:185-192; small.yml.j2:73-87) + L2 regulariser gradient."""
        o = self.optimizer
        self._gradient_noise()  # gradn_config (base_model.py:185-191): no-op unless compiled with one
        self.step += 1
        # keras evaluates the schedule at `iterations` BEFORE the increment (0 at the first update: the reference's first step has
        # lr = 0 with TransformerSchedule) and bias-corrects with iterations + 1 [ext: keras BaseOptimizer._get_current_learning_rate,
        # Adam.update_step]
        lr = self.learning_rate(self.step - 1)
        ps = self.ps
        # bf16 models: the optimizer writes the bf16 shadow of the parameters itself
        fused = ps.shadow is not ps.flat and ps.shadow.dtype == torch.bfloat16
        K.adam(ps.flat, ps.grad, ps.adam_m, ps.adam_v, ps.n_reg, lr, self.step, o["beta1"], o["beta2"], o["eps"], o["weight_decay"],
               self.cfg.l2, grad_scale, shadow=ps.shadow if fused else None)
        if not fused:
            ps.refresh_shadow()
        return lr

    def regularization_loss(self):
        out = torch.zeros(1, dtype=torch.float32, device=self.device)
        K.sumsq(self.ps.flat, self.ps.n_reg, out)
        return out * self.cfg.l2

    def train_step(self, data: TrainData, masks=None):
        """BaseModel.train_step / train_step_ga (base_model.py:194-209): returns {'loss': per-utterance costs [B]}.
        With ga_steps > 1 the optimizer is applied every ga_steps-th call with (sum of micro-grads)/ga_steps
        (optimizers/accumulation.py:64-70)."""
        if self._ga_count == 0:
            self.zero_grad()
        # the flat buffer accumulates LOCAL micro-gradients; it is all-reduced once, on the apply micro-step, where the
        # bucketed slices still overlap that micro-step's backward (base_model.py:200-209)
        original_weights = self.apply_gwn()  # gwn_config (base_model.py:156-159): no-op unless compiled with one
        costs = self.loss_and_backward(data, True, masks, reduce=self._ga_count + 1 >= self.ga_steps)
        self.remove_gwn(original_weights)
        self._ga_count += 1
        if self._ga_count >= self.ga_steps:
            self.apply_gradients(1.0 / self.ga_steps)
            self._ga_count = 0
        return {"loss": costs}

    def get_initial_tokens(self, batch_size=1):
        return torch.full((batch_size, 1), self.blank, dtype=torch.int32, device=self.device)

    def inference_twin(self):
        """This model in f32 parity mode over the SAME parameter buffers (f32 master weights, BatchNorm moving statistics): no copy,
        always current.  The twin of an f32 model is the model itself."""
        if self.dtype == torch.float32:
            return self
        if self._twin is None:
            t = object.__new__(type(self))
            t.__dict__.update(self.__dict__)
            t.dtype, t.ps = torch.float32, self.ps.alias(torch.float32)
            t._twin = None
            t._reset_caches()  # (everything else is shared: streams, switches, an inference-only encoder's `_derived`, keyed by type)
            t.timers, t.timer_work = None, {}
            self._twin = t
        return self._twin

    @torch.no_grad()
    def encode(self, signals, signals_length, precision=None):
        """frontend + ConformerEncoder.call_next (conformer.py:703-718), inference mode (moving BN statistics).
        precision "f32" (default, self.decode_precision) runs it on the f32 master weights; "bf16" on the training kernels."""
        if (precision or self.decode_precision) == "f32" and self.dtype != torch.float32:
            return self.inference_twin().encode(signals, signals_length)
        sig = signals.to(self.device, non_blocking=True)
        slen = [int(v) for v in signals_length.tolist()]
        feats, flen = self.frontend(sig, slen, training=False)
        enc, T, elen, _ = self.encoder_fwd(feats, flen, False, None)
        return enc.view(sig.shape[0], T, self.cfg.dmodel), elen

    @property
    def seconds_per_frame(self):
        return self.cfg.time_reduction_factor * self.cfg.stride_ms / 1000.0

    # =================================================================================== streaming (streaming.py, csrc/stream.hip)
    def stream_state(self, batch_size=1, precision=None):
        """Encoder state of `batch_size` streams for encode_chunk (the class streaming.STREAM_STATES names for the encoder, after its refusal
        rule).  precision as encode: "f32" (default) = the inference twin."""
        from . import streaming

        return streaming.check_streamable(self)(streaming._twin(self, precision), batch_size)

    def encode_chunk(self, state, feats, nframes, final=()):
        """One step of the streaming encoder (the state's `encode`): feats [B, n, F] (the Conformer: n <= 4 chunk_size), nframes [B], final
        = the streams that end with these frames (RnntStreamState) -> (enc [B, rows, dmodel] (the Conformer: chunk_size rows), nvalid [B])."""
        from . import streaming

        if not isinstance(state, streaming.check_streamable(self)):
            raise ValueError("encoder state of another model")
        return streaming.encode_chunk(state, feats, nframes, final)

    def stream_detailed(self, *args, **kwargs):
        """stream(...) of this class with the same arguments, opened as a detail session (greedy only; a beam raises ValueError): the
        outputs also say when each token was spoken and how sure the model was (streaming.StreamDetailOutput, rec.recognized(),
        DESIGN.md 4b-3).  One method for every streamable class: their stream() signatures differ and stay as they are."""
        return self.stream(*args, **kwargs).detailed()

    def stream_horizon(self, commit_horizon, *args, **kwargs):
        """stream(...) of this class with the same arguments (beam_width >= 1 among them), opened with a commit horizon of
        `commit_horizon` encoder frames: an endless beam session whose committed text trails the audio by about the horizon, at the
        price of a pruning rule (streaming.StreamingRecognizer).  One method for every streamable class, as
        stream_detailed: their stream() signatures differ and stay as they are."""
        lm = {k: kwargs.pop(k) for k in ("lm", "lm_alpha", "lm_beta") if k in kwargs}  # (stream_lm's keywords, accepted here too)
        if lm.get("lm") is not None:
            return self.stream_lm(lm.pop("lm"), *args, **lm, **kwargs).with_commit_horizon(commit_horizon)
        return self.stream(*args, **kwargs).with_commit_horizon(commit_horizon)

    def stream_lm(self, lm, *args, lm_alpha=0.5, lm_beta=0.0, **kwargs):
        """stream(...) of this class with the same arguments (1 <= beam_width <= 32 among them), opened with the n-gram model `lm`
        (lm.NGramLM) fused into the carried CTC beam: the beam of recognize_nbest_lm(alpha=lm_alpha, beta=lm_beta), carried from chunk
        to chunk, on the model's own blank self.blank - not the V-1 convention of the plain beam session (streaming.StreamingRecognizer,
        DESIGN.md 4b-4).  lm=None: stream(...) itself.  One method for every streamable class, as stream_horizon: their stream()
        signatures differ and stay as they are.  A transducer head raises NotImplementedError; beam_width 0 or > 32 and a detail
        session ValueError - judged from the arguments, before the session is opened."""
        if lm is not None:
            import inspect

            from . import streaming

            bound = inspect.signature(self.stream).bind(*args, **kwargs)
            bound.apply_defaults()
            streaming.check_stream_lm(self, lm, lm_alpha, lm_beta, bound.arguments.get("beam_width", 0))
        return self.stream(*args, **kwargs).with_lm(lm, lm_alpha, lm_beta)

    # ----------------------------------------------------------------- timing hooks (bench.py)
    def _tick(self, name):
        if self.timers is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def _tock(self, name, start, work=0.0):
        if self.timers is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.timers.setdefault(name, []).append((start, e))
        self.timer_work.setdefault(name, []).append(work)


def _mel_weight_matrix(num_mel_bins, num_spectrogram_bins, sample_rate, lower, upper):
    """tf.signal.linear_to_mel_weight_matrix semantics (feature_extraction.py:222-229): HTK mel scale, DC row zero,
    un-normalised triangles, float32 arithmetic."""
    f32 = np.float32

    def mel(f):
        return (f32(1127.0) * np.log(f32(1.0) + np.asarray(f, f32) / f32(700.0))).astype(f32)

    nyquist = f32(sample_rate) / f32(2.0)
    linear = np.linspace(f32(0.0), nyquist, num_spectrogram_bins, dtype=f32)[1:]
    spec_mel = mel(linear)[:, None]
    edges = np.linspace(mel(lower), mel(upper), num_mel_bins + 2, dtype=f32)
    lo, ce, hi = edges[:-2][None, :], edges[1:-1][None, :], edges[2:][None, :]
    w = np.maximum(f32(0.0), np.minimum((spec_mel - lo) / (ce - lo), (hi - spec_mel) / (hi - ce))).astype(f32)
    return np.pad(w, [[1, 0], [0, 0]]).astype(f32)
