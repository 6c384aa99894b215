"""Incremental recognition with the streaming Conformer (chunked attention mask, causal convolutions): chunk-by-chunk encoder with
state carried on the device, and the searches (greedy, or a beam carried whole) continued across chunks.

The contract ("Streaming"): stream b of a session produces the encoder frames and the tokens that `model.encode` /
`model.recognize` produce for that utterance run ALONE (batch size 1), however the samples arrive and whatever the other streams of the
session do.  State carried per stream:
    frontend      unconsumed samples (host side, < frame_length + frame_step + one chunk) and the last consumed raw sample
    subsampling   the last 2 feature frames and the last 2 frames of the first convolution's activation (zeros = the causal padding)
    each block    K and V of the last `history_size` frames (rings), the last kernel_size - 1 GLU outputs of the conv module
    search        last token, LSTM h / c (transducer); the class of the last frame (CTC); a detail session's CTC head carries
                  K.CtcDetailState instead (that class, the frames seen, the open token's start and sums, the path score)
    beam search   (beam_width >= 1) the whole beam: rows, f64 totals, label trie + table, prediction states (K.RnntBeamStream); the
                  CTC search's rows and trie (K.CtcBeamStream); the depth committed so far
The kernels that touch carried state are csrc/stream.hip; the dense pieces are the forward kernels of training with T = chunk_size.
Everything the session knows about an encoder is EncoderStream, the base of the five state classes (STREAM_STATES: cfg.encoder -> class).
A Transformer with a chunked config streams under the same contract (TransformerStreamState, transformer_encode_chunk): its blocks carry
the K / V rings only (there is no convolution module), the absolute position rows are taken at each stream's own offset, and the ring
append is part of the attention launch.
The unidirectional DeepSpeech2 (causal Conv2D, forward LSTMs, causal RowConv1D) streams under the same contract (DS2StreamState,
ds2_encode_chunk): it carries the last kh - 1 input rows of every conv block, each LSTM's (h, c) and the last K - 1 input rows of every
RowConv1D.
The RNN-Transducer (LSTM encoder with time reductions) streams under the same contract (RnntStreamState, rnnt_encode_chunk): it carries
each block's LSTM (h, c) and, in front of every time reduction, the fewer-than-factor rows that do not fill a group yet.
"""
import math
import typing

import numpy as np
import torch

from . import kernels as K
from .base_model import BaseModel
from .kernels import ACT_SWISH
from .params import rnnt_modules
from .rnnt import boundary_factors


class StreamOutput(typing.NamedTuple):
    tokens: torch.Tensor  # [B, W] int32 on the host: the tokens NEW in this call, blank padded
    tokens_length: torch.Tensor  # [B] int32
    frames: torch.Tensor  # [B] int32: encoder frames emitted so far


class StreamDetailOutput(typing.NamedTuple):
    """What a detail session (model.stream_detailed) returns: StreamOutput's three fields, then the time and the confidence of every token of the
    call, column-aligned with `tokens` (-1 / 0 where no token sits).  Frames count from the stream's reset."""
    tokens: torch.Tensor
    tokens_length: torch.Tensor
    frames: torch.Tensor
    token_frames: torch.Tensor  # [B, W] int32: transducer = the encoder frame whose decision emitted the token; CTC = the first frame of its run
    token_ends: typing.Optional[torch.Tensor]  # [B, W] int32, CTC only: one past the run's last frame, -1 while the run is open; None for the transducer
    log_probs: torch.Tensor  # [B, W] f32 (CTC: summed over the run; over its frames so far while it is open)
    entropies: torch.Tensor  # [B, W] f32 (CTC: mean over the run; over its frames so far while it is open)


def _refuse(model, why):
    """the refusal of the inference-only models, in the words of their other refusals ("inference only") followed by the reason"""
    raise NotImplementedError(f"{type(model).__name__} is inference only, and this configuration cannot be streamed: {why}")


def _frame_counts(model, feats, nframes, keep_device=False, upload=True):
    """nframes [B], the feature frames of feats [B, n, F] that are real per stream -> (host list, device int32 vector - None without
    `upload`); B counts in 0 .. n or ValueError.  keep_device: a tensor goes to the device as it is, without being read back (host list
    None, no range check)."""
    if keep_device and isinstance(nframes, torch.Tensor):
        return None, nframes.to(model.device).to(torch.int32).contiguous()
    host = [int(v) for v in (nframes.tolist() if isinstance(nframes, torch.Tensor) else nframes)]
    if len(host) != feats.shape[0] or min(host) < 0 or max(host) > feats.shape[1]:
        raise ValueError(f"encode_chunk takes B = {feats.shape[0]} frame counts within its {feats.shape[1]} feature frames")
    return host, model._h2d(host) if upload else None


class EncoderStream:
    """Encoder state of `batch_size` streams, and everything a session (StreamingRecognizer) knows about the encoder; what a new encoder
    supplies to stream ("The encoder-stream interface"):
        check(model)                   the refusal rule: raises, with the reason, for a config that cannot stream (check_streamable)
        step_rule(cfg, chunk_frames)   host only -> (feature frames of a step, encoder rows of a step's output buffer, reduce(t) = the
                                       encoder frames of t feature frames); ValueError for a chunk_frames the encoder cannot take
        f32_features, prepare(feats)   the front end writes f32 (else the compute type); what happens to its output before the encoder
        encode(feats, nframes, final)  one step -> (enc [B, rows, dmodel], nvalid [B] int32 device, nvalid host list); advances the state
        uses_final                     the encoder carries rows that only a final step sends out (`final` = the streams that end here)
        reset / export / load          here, over _tensors() (the carried device tensors) and the _host_* hooks (counters on the host)"""
    f32_features = False
    uses_final = False
    host_tensors = 0  # tensors export() appends to the carried ones for the state kept on the host

    def __init__(self, model, batch_size):
        self.check(model)
        self.model, self.B = model, int(batch_size)

    @staticmethod
    def check(model):
        pass

    def prepare(self, feats):
        return feats

    def _reduced(self, host):
        return None if host is None else [self.model._encoder_length(t) for t in host]

    _host_reset = _host_load = lambda self, arg: None  # hooks: reset(rows) and load(what _host_export appended) of state kept on the host
    _host_export = lambda self: []

    def reset(self, rows=None):
        for t in self._tensors():
            if rows is None:
                t.zero_()
            else:
                t[torch.as_tensor(list(rows), dtype=torch.long, device=t.device)] = 0
        self._host_reset(range(self.B) if rows is None else rows)

    def export(self):
        """The carried tensors as one flat list (a copy): what PredictOutput.next_encoder_states holds."""
        return [t.clone() for t in self._tensors()] + self._host_export()

    def load(self, tensors):
        mine = self._tensors()
        if len(tensors) != len(mine) + self.host_tensors:
            raise ValueError("encoder state of another model")
        for a, b in zip(mine, tensors):
            a.copy_(b)
        self._host_load(tensors[len(mine):])


def _chunked_step(cfg, chunk_frames, reduce):
    """the step of the chunked-attention encoders: 4 * chunk_size feature frames -> chunk_size encoder frames"""
    if chunk_frames is not None:
        raise ValueError("stream: chunk_frames belongs to the Jasper and DeepSpeech2 sessions; a Conformer's step is 4 * chunk_size "
                         "feature frames")
    return 4 * int(cfg.chunk_size), int(cfg.chunk_size), reduce


def _strided_step(cfg, chunk_frames=None, most=None, limit=""):
    """the step of the strided causal encoders: `chunk_frames` feature frames -> chunk_frames / factor encoder frames (a stream's last
    step: ceil of what is left), `most` rows at the most"""
    factor = int(cfg.time_reduction_factor)
    n = int(chunk_frames if chunk_frames is not None else 32)
    if n < factor or n % factor:
        raise ValueError(f"stream: chunk_frames {n} must be a positive multiple of the time reduction factor {factor}")
    if most is not None and n // factor > most:
        raise ValueError(f"stream: chunk_frames {n} is more than {most} encoder frames a step ({limit})")
    return n, n // factor, cfg.encoder_length


@torch.no_grad()
def _causal_stem(state, feats, nframes, conv_norm1, conv_norm2, keep_device=False):
    """The causal two-convolution subsampling of one step with its two carries: feats [B, n <= 4C, F] -> (x [B*C, dmodel], frame counts
    on the host, nvalid [B] int32 device).  conv_norm1(carry ++ rows [B, 4C + 2, F]) -> [B, 2C + 1, F1, C0] and conv_norm2(im2col rows)
    -> [B (C + 1) F2, C1] are the model's convolution + norm pairs."""
    m = state.model
    c, ps, dev = m.cfg, m.ps, m.device
    B, C = state.B, int(c.chunk_size)
    n0 = 4 * C
    if feats.shape[0] != B or feats.shape[1] > n0:
        raise ValueError(f"encode_chunk takes [B = {B}, <= {n0}, F] feature frames")
    host, nf = _frame_counts(m, feats, nframes, keep_device)
    cat = torch.zeros(B, n0 + 2, c.num_feature_bins, dtype=m.dtype, device=dev)
    cat[:, :2] = state.feat_carry
    cat[:, 2:2 + feats.shape[1]] = feats
    n1 = (nf + 1) // 2
    nvalid = ((n1 + 1) // 2).to(torch.int32).contiguous()
    two = torch.arange(2, device=dev)
    # the carries move to the last two VALID rows (rows nf, nf + 1 of carry ++ new; nf == 0 picks the carry itself)
    idx = (nf.long()[:, None] + two[None, :])
    state.feat_carry.copy_(torch.gather(cat, 1, idx[:, :, None].expand(B, 2, cat.shape[2])))
    # causal 3x3 stride-2 convs on carry(2) ++ new(n): output 0 belongs to the previous chunk, outputs 1.. are the originals
    a1 = conv_norm1(cat)
    F1, C0 = a1.shape[2], a1.shape[3]
    cat1 = torch.cat([state.conv_carry, a1[:, 1:]], 1).contiguous()  # [B, 2C + 2, F1, C0]
    idx1 = (n1.long()[:, None] + two[None, :])
    state.conv_carry.copy_(torch.gather(cat1, 1, idx1[:, :, None, None].expand(B, 2, F1, C0)))
    a2 = conv_norm2(K.im2col_3x3s2(cat1))
    merged = a2.view(B, C + 1, -1)[:, 1:].reshape(B * C, -1)
    return K.matmul(merged, ps.w2d("enc/linear/w"), bias=ps.p("enc/linear/b")), host, nvalid


class StreamState(EncoderStream):
    """Encoder state of `batch_size` Conformer streams (device tensors) plus the per-layer constant position tables."""

    def __init__(self, model, batch_size):
        super().__init__(model, batch_size)
        c, ps, dev, dt = model.cfg, model.ps, model.device, model.dtype
        B, C, hist = self.B, int(c.chunk_size), int(c.history_size)
        HD = c.num_heads * ps.head_phys
        F1 = (c.num_feature_bins + 1) // 2
        self.seen = torch.zeros(B, dtype=torch.int32, device=dev)
        self.feat_carry = torch.zeros(B, 2, c.num_feature_bins, dtype=dt, device=dev)
        self.conv_carry = torch.zeros(B, 2, F1, ps.filt_phys, dtype=dt, device=dev)
        nb = c.num_blocks
        self.kcache = [torch.zeros(B, hist, HD, dtype=dt, device=dev) for _ in range(nb)]
        self.vcache = [torch.zeros(B, hist, HD, dtype=dt, device=dev) for _ in range(nb)]
        self.dwstate = [torch.zeros(B, c.kernel_size - 1, c.dmodel, dtype=dt, device=dev) for _ in range(nb)]
        # alone, key j seen from query i sits at position i - j in [-(C-1), hist + C - 1]: one constant table per layer
        pos = np.arange(hist + C - 1, -C, -1).astype(np.float32)
        d = c.dmodel
        ts = np.power(np.float32(1.0 / 10000.0), (2 * (np.arange(d, dtype=np.float32) // 2)) / np.float32(d)).astype(np.float32)
        ang = pos[:, None] * ts[None, :]
        pe = np.where((np.arange(d) % 2 == 1)[None, :], np.cos(ang), np.sin(ang)).astype(np.float32)
        pe = torch.from_numpy(pe).to(dev).to(dt).contiguous()
        self.pext = [K.matmul(pe, ps.w2d(f"enc/block{i}/mhsa/pos/w"), bias=ps.p(f"enc/block{i}/mhsa/pos/b")) for i in range(nb)]

    @staticmethod
    def check(model):
        c = model.cfg
        if c.chunk_size is None:
            raise ValueError("streaming needs a streaming config: chunk_size is None (full-context attention sees the whole utterance)")
        if c.history_size is None or int(c.history_size) < 0:
            raise ValueError("streaming needs history_size >= 0: unlimited history would need an unbounded key / value cache")
        C, hist = int(c.chunk_size), int(c.history_size)
        if C < 1 or C > K.STREAM_MAX_CHUNK or hist + C > K.STREAM_MAX_KEYS or model.ps.head_phys > K.STREAM_MAX_HEAD or c.kernel_size > 32:
            raise ValueError(f"chunk_size {C} / history_size {hist} / head {model.ps.head_phys} / kernel {c.kernel_size} beyond the streaming "
                             f"kernels' limits (chunk <= {K.STREAM_MAX_CHUNK}, history + chunk <= {K.STREAM_MAX_KEYS}, head <= "
                             f"{K.STREAM_MAX_HEAD}, kernel <= 32)")

    @staticmethod
    def step_rule(cfg, chunk_frames=None):
        return _chunked_step(cfg, chunk_frames, BaseModel._encoder_length)

    def _tensors(self):
        return [self.seen, self.feat_carry, self.conv_carry] + self.kcache + self.vcache + self.dwstate

    @torch.no_grad()
    def encode(self, feats, nframes, final=()):
        """One encoder step: feats [B, n <= 4C, F] (compute dtype, device), nframes [B] int32 feature frames that are real per stream: 0
        (idle), 4C (a full chunk) or in between for a stream's last chunk -> (enc [B, C, dmodel], nvalid [B] int32 device, nvalid on the
        host - None for a device tensor of counts, which is not read back); advances state."""
        m = self.model
        c, ps = m.cfg, m.ps
        B, C, hist = self.B, int(c.chunk_size), int(c.history_size)
        H, dh, d = c.num_heads, ps.head_phys, c.dmodel
        Cp = ps.filt_phys

        def conv_norm1(cat):
            c1 = K.conv1_fwd(cat, ps.p("enc/sub/conv0/w"), ps.p("enc/sub/conv0/b"))  # [B, 2C + 1, F1, Cp]
            return m._sub_norm_fwd(c1.view(-1, Cp), "enc/sub/bn0", False)[0].view(c1.shape)

        def conv_norm2(col):
            return m._sub_norm_fwd(K.matmul(col, ps.w2d("enc/sub/conv1/w"), bias=ps.p("enc/sub/conv1/b")), "enc/sub/bn1", False)[0]

        x, host, nvalid = _causal_stem(self, feats, nframes, conv_norm1, conv_norm2, keep_device=True)
        scale = 1.0 / math.sqrt(c.head_size)
        for i in range(c.num_blocks):
            p = f"enc/block{i}/"
            x = m._ffm_fwd(x, p + "ff1/", None, 0, False)
            pfx = p + "mhsa/"
            ln, _, _ = K.layernorm_fwd(x, ps.p(pfx + "ln/g"), ps.p(pfx + "ln/b"))
            qkv = K.matmul(ln, ps.w2d(pfx + "qkv/w"), bias=ps.p(pfx + "qkv/b"))
            ub, vb = m._uv(pfx)
            att = K.stream_attn_fwd(qkv, ub, vb, self.pext[i], self.kcache[i], self.vcache[i], self.seen, nvalid, B, C, H, dh, hist, scale)
            K.stream_kv_append(qkv, self.kcache[i], self.vcache[i], self.seen, nvalid, B, C, H, dh, hist)  # after every head has read the ring
            x = K.matmul(att, ps.w2d(pfx + "o/w"), bias=ps.p(pfx + "o/b"), res=x, beta=c.mhsam_residual)
            pfx = p + "conv/"
            ln, _, _ = K.layernorm_fwd(x, ps.p(pfx + "ln/g"), ps.p(pfx + "ln/b"))
            a = K.matmul(ln, ps.w2d(pfx + "pw1/w"), bias=ps.p(pfx + "pw1/b"))
            cv = K.stream_glu_dwconv_fwd(a, self.dwstate[i], ps.p(pfx + "dw/w"), ps.p(pfx + "dw/b"), nvalid, B, C)
            if c.convm_dw_norm == "layer":
                yn, _, _ = K.layernorm_fwd(cv, ps.p(pfx + "bn/g"), ps.p(pfx + "bn/b"))
                sw = K.add_act_fwd(yn, None, ACT_SWISH)
            else:
                sw, _ = m._bn_fwd(cv, pfx + "bn", False, ACT_SWISH)
            x = K.matmul(sw, ps.w2d(pfx + "pw2/w"), bias=ps.p(pfx + "pw2/b"), res=x, beta=c.convm_residual)
            x = m._ffm_fwd(x, p + "ff2/", None, 0, False)
            x, _, _ = K.layernorm_fwd(x, ps.p(p + "ln/g"), ps.p(p + "ln/b"))
        self.seen += nvalid
        return x.view(B, C, d), nvalid, self._reduced(host)


class TransformerStreamState(EncoderStream):
    """Encoder state of `batch_size` Transformer streams: seen, the last 2 feature frames, the last 2 rows of the first convolution
    block's activation (after the folded BatchNorm and the ReLU), one K and one V ring [B, history_size, H * head_size] per block.  The
    absolute position table [Tcap, dmodel] f32 is a constant, not state: its rows depend on the position only, so it is grown by doubling
    (from the frame counters kept on the host) before a launch would pass its end, and it is not exported."""

    def __init__(self, model, batch_size):
        super().__init__(model, batch_size)
        c, dev, dt = model.cfg, model.device, model.dtype
        B, hist, HD = self.B, int(c.history_size), int(c.num_heads) * int(c.head_size)
        F1 = (c.num_feature_bins + 1) // 2
        self.seen = torch.zeros(B, dtype=torch.int32, device=dev)
        self.feat_carry = torch.zeros(B, 2, c.num_feature_bins, dtype=dt, device=dev)
        self.conv_carry = torch.zeros(B, 2, F1, int(c.sub_filters[0]), dtype=dt, device=dev)
        nb = int(c.num_blocks)
        ring = lambda: torch.zeros(B, hist, HD, dtype=dt, device=dev) if hist > 0 else None
        self.kcache, self.vcache = [ring() for _ in range(nb)], [ring() for _ in range(nb)]
        self.host_seen = [0] * B  # encoder frames per stream, as the device vector `seen` holds them
        self.pe = None
        self.reserve(4 * int(c.chunk_size))

    @staticmethod
    def check(model):
        """A Transformer streams when its attention mask is the chunked one (use_attention_auto_mask, chunk_size, history_size >= 0) and
        the sizes fit tfasr_stream_attn_plain_fwd; the causal flag is allowed (the kernel has it)."""
        c = model.cfg
        if c.chunk_size is None:
            _refuse(model, "chunk_size is None (full-context attention sees the whole utterance)")
        if not c.use_attention_auto_mask:
            _refuse(model, "use_attention_auto_mask is off (no mask is computed: every frame attends over the whole utterance)")
        if c.history_size is None or int(c.history_size) < 0:
            _refuse(model, "unlimited history would need an unbounded key / value cache")
        C, hist, dh = int(c.chunk_size), int(c.history_size), int(c.head_size)
        if C < 1 or C > K.STREAM_MAX_CHUNK or hist + C > K.STREAM_MAX_KEYS or dh > K.STREAM_MAX_HEAD:
            _refuse(model, f"chunk_size {C} / history_size {hist} / head {dh} beyond the streaming kernels' limits (chunk <= "
                           f"{K.STREAM_MAX_CHUNK}, history + chunk <= {K.STREAM_MAX_KEYS}, head <= {K.STREAM_MAX_HEAD})")

    @staticmethod
    def step_rule(cfg, chunk_frames=None):  # the Conformer's step and frame reduction
        return _chunked_step(cfg, chunk_frames, cfg.encoder_length)

    def reserve(self, rows):
        """the position table covers positions 0 .. rows - 1 at least"""
        cap = 0 if self.pe is None else self.pe.shape[0]
        if rows <= cap:
            return
        cap = max(cap, 256)
        while cap < rows:
            cap *= 2
        from .transformer import sinusoid_table

        c = self.model.cfg
        self.pe = torch.from_numpy(sinusoid_table(cap, c.dmodel, bool(c.interleave_relpe))).to(self.model.device).contiguous()

    def _tensors(self):
        return [self.seen, self.feat_carry, self.conv_carry] + [t for t in self.kcache + self.vcache if t is not None]

    def _host_reset(self, rows):
        for b in rows:
            self.host_seen[b] = 0

    def _host_load(self, tensors):
        self.host_seen = [int(v) for v in self.seen.tolist()]

    @torch.no_grad()
    def encode(self, feats, nframes, final=()):
        """One step of the streaming Transformer encoder: feats [B, n <= 4C, F] (compute dtype, device), nframes [B] feature frames that
        are real per stream (0 = idle, 4C = a full chunk, fewer for a stream's last chunk) -> (enc [B, C, dmodel], nvalid [B] int32
        device, nvalid on the host); advances state.  The subsampling is the Conformer's on this model's layers (_causal_stem), the position
        rows are those of each stream's own offset (tfasr_stream_add_pe), and a block is TransformerEncoderMixin.block_fwd at T = C around
        tfasr_stream_attn_plain_fwd, which also appends the chunk's keys and values to the rings."""
        m = self.model
        c, ps = m.cfg, m.ps
        B, C, hist = self.B, int(c.chunk_size), int(c.history_size)
        H, dh, d = int(c.num_heads), int(c.head_size), int(c.dmodel)
        c0, c1 = m.modules["convs"]

        def conv_norm1(cat):
            a1 = K.conv1_fwd(cat, ps.p(c0["name"] + "/w"), ps.p(c0["name"] + "/b"))  # [B, 2C + 1, F1, C0]
            return K.channel_affine_fwd(a1, *m._affine(c0["bn"]), relu=True, y=a1)

        def conv_norm2(col):
            a2 = K.matmul(col, ps.w2d(c1["name"] + "/w"), bias=ps.p(c1["name"] + "/b"))
            return K.channel_affine_fwd(a2, *m._affine(c1["bn"]), relu=True, y=a2)

        x, host, nvalid = _causal_stem(self, feats, nframes, conv_norm1, conv_norm2)
        nv_host = self._reduced(host)
        seen = [s + n for s, n in zip(self.host_seen, nv_host)]
        self.reserve(max(seen))
        x = K.stream_add_pe(x.view(B, C, d), self.pe, self.seen, nvalid).view(B * C, d)
        scale, causal = 1.0 / math.sqrt(dh), bool(c.use_attention_causal_mask)
        for i, p in enumerate(m.modules["blocks"]):
            attend = lambda qkv, i=i: K.stream_attn_plain_fwd(qkv, self.kcache[i], self.vcache[i], self.seen, nvalid, B, C, H, dh, hist, scale, causal)
            x = m.block_fwd(x, p, B, C, None, i, attend=attend)
        self.seen += nvalid
        self.host_seen = seen
        return x.view(B, C, d), nvalid, nv_host


class JasperStreamState(EncoderStream):
    """Encoder state of `batch_size` Jasper streams: per Conv1D layer with more than one tap, the last (K - 1) * dilation rows of its
    input, [B, (K - 1) * dilation, Cin] in the compute type (zeros = the causal padding of a stream's start).  Causal convolutions only:
    every config streams exactly."""
    f32_features = True

    def __init__(self, model, batch_size):
        super().__init__(model, batch_size)
        self.tails = [torch.zeros(self.B, (m["K"] - 1) * m["dilation"], m["cin"], dtype=model.dtype, device=model.device) if m["K"] > 1 else None
                      for m in model.layers]

    step_rule = staticmethod(_strided_step)

    def prepare(self, feats):
        return self.model._scale_feats(feats)

    def _tensors(self):
        return [t for t in self.tails if t is not None]

    @torch.no_grad()
    def encode(self, feats, nframes, final=()):
        """One encoder step: feats [B, n, F] (compute type, device), nframes [B] feature frames that are real per stream (0 = idle; n; fewer
        for a stream's last step; even everywhere else when the first block strides by 2) -> (enc [B, ceil(n / factor), dmodel], nvalid [B]
        int32 device, nvalid on the host - None for a device tensor of counts, which is not read back); advances state.  Each layer
        convolves [tail | rows] with the tail as real left context (tfasr_conv1d_fwd's `lead`), then the tail moves to the last rows that
        are valid for the stream (tfasr_conv1d_tail_update)."""
        m = self.model
        if feats.shape[0] != self.B:
            raise ValueError(f"encode_chunk takes [B = {self.B}, n, F] feature frames")
        host, nv = _frame_counts(m, feats, nframes, keep_device=True)
        x, residuals, starts = feats.contiguous(), [], m._block_starts()
        for li, mod in enumerate(m.layers):
            if li in starts:
                residuals.append(x)
            tail = self.tails[li]
            if tail is None:
                x = m._layer_fwd(x, mod, residuals)
            else:
                win = torch.cat([tail, x], 1)
                x = m._layer_fwd(win, mod, residuals, lead=tail.shape[1])
                K.conv1d_tail_update(win, nv, tail)
            if mod["stride"] > 1:
                nv = ((nv + (mod["stride"] - 1)) // mod["stride"]).to(torch.int32).contiguous()
        return x, nv, self._reduced(host)


PERSIST_STREAMS = 64  # tfasr_lstm_infer_fwd's persistent launch takes up to 64 batch rows


class _CarriedLstm:
    """h and c [B, P] f32 (h holds numbers of the compute type) of a stack of forward LSTMs, carried from step to step.  The recurrence
    reads one (h, c) pair and writes another (the library refuses aliases: tfasr_lstm_infer_fwd_state), so every layer owns two pairs and
    `cur` says which one holds the state; tensors() / reference_states() speak of that one only."""

    def __init__(self, model, batch_size, units):
        self.hc = [[tuple(torch.zeros(batch_size, P, dtype=torch.float32, device=model.device) for _ in range(2)) for _ in range(2)] for P in units]
        self.cur = [0] * len(self.hc)
        # in bf16 more than 64 streams run the recurrence in slices of 64: every slice stays on the persistent launch, the route the
        # utterance alone takes (the per-step route rounds differently)
        self.slice = PERSIST_STREAMS if model.dtype != torch.float32 else batch_size

    def tensors(self):
        return [t for pairs, cur in zip(self.hc, self.cur) for t in pairs[cur]]

    def reference_states(self):
        """[B, nlayers, 2, P] f32, states ordered (h, c): what the reference's encoders exchange through get_initial_state / call_next
        (DeepSpeech2Encoder; RnnTransducerEncoder, encoders/rnnt.py:171-211)"""
        return torch.stack([torch.stack(list(pairs[cur]), 1) for pairs, cur in zip(self.hc, self.cur)], 1)

    def run(self, li, xg, rk, lens):
        """layer li's recurrence over xg [B, T, 4P] for lens [B] rows per stream, continued from the carried state -> y [B, T, P]"""
        B, T, P = xg.shape[0], xg.shape[1], xg.shape[2] // 4
        (h0, c0), (h1, c1) = self.hc[li][self.cur[li]], self.hc[li][self.cur[li] ^ 1]
        y = torch.empty(B, T, P, dtype=xg.dtype, device=xg.device)
        for b0 in range(0, B, self.slice):
            e = min(b0 + self.slice, B)
            K.lstm_infer_fwd(xg[b0:e], rk, lens[b0:e], y=y[b0:e], state=(h0[b0:e], c0[b0:e]), state_out=(h1[b0:e], c1[b0:e]))
        self.cur[li] ^= 1
        return y


class DS2StreamState(EncoderStream):
    """Encoder state of `batch_size` streams of the unidirectional DeepSpeech2.  Per stream:
        each conv block   the last kh - 1 rows of its input, [kh - 1, F_in * Cin] in the compute type (zeros = the causal padding)
        each RnnBlock     h and c [P] f32 (_CarriedLstm), and with a RowConv1D the last K - 1 rows of the LSTM's output, [K - 1, P] in the
                          compute type"""
    f32_features = True

    def __init__(self, model, batch_size):
        super().__init__(model, batch_size)
        B, dev, dt, mods = self.B, model.device, model.dtype, model.modules
        shapes = model.cfg.conv_shapes()
        self.conv_tails = [torch.zeros(B, kh - 1, fi * ci, dtype=dt, device=dev) if kh > 1 else None for kh, _kw, ci, _co, _st, _sf, fi, _fo in shapes]
        self.lstm = _CarriedLstm(model, B, [r["P"] for r in mods["rnns"]])
        self.row_tails = [torch.zeros(B, r["K"] - 1, r["P"], dtype=dt, device=dev) if r["rowconv"] and r["K"] > 1 else None for r in mods["rnns"]]

    @staticmethod
    def check(model):
        """A DeepSpeech2 streams when it is causal throughout: forward LSTMs only and causal convolutions."""
        c = model.cfg
        if c.rnn_bidirectional:
            _refuse(model, "rnn_bidirectional (the backward direction starts at the utterance's last frame)")
        if c.conv_padding != "causal":
            _refuse(model, f"conv_padding = {c.conv_padding!r} (a 'same'-padded convolution reads frames that have not arrived yet)")

    @staticmethod
    def step_rule(cfg, chunk_frames=None):
        return _strided_step(cfg, chunk_frames, K.STREAM_MAX_CHUNK, "tfasr_stream_rowconv_fwd's limit")

    def reference_states(self):
        return self.lstm.reference_states()

    def prepare(self, feats):  # DeepSpeech2CTC.frontend's route: f32 out of the kernel, then the cast
        dt = self.model.dtype
        return feats if dt == torch.float32 else K.cast(feats, torch.empty(feats.shape, dtype=dt, device=feats.device))

    def _tensors(self):
        return [t for t in self.conv_tails if t is not None] + self.lstm.tensors() + [t for t in self.row_tails if t is not None]

    @torch.no_grad()
    def encode(self, feats, nframes, final=()):
        """One encoder step of the unidirectional DeepSpeech2: feats [B, n, F] (compute type, device; n a multiple of the time reduction
        factor), nframes [B] feature frames that are real per stream (0 = idle; n; fewer for a stream's last step) -> (enc [B, n / factor,
        dmodel], nvalid [B] int32 device, reduced over the time strides as cfg.encoder_length does, nvalid on the host); advances state.
        Each conv block convolves [tail | rows] with the tail as real left context (conv2d_fwd's `lead`), then the tail moves to the last
        rows valid for the stream; each RnnBlock is one GEMM, one recurrence continued from the carried state (_CarriedLstm.run, lengths =
        the valid rows) and one tfasr_stream_rowconv_fwd; then the FC blocks."""
        m = self.model
        c, B = m.cfg, self.B
        factor = int(c.time_reduction_factor)
        if feats.dim() != 3 or feats.shape[0] != B or feats.shape[1] < factor or feats.shape[1] % factor:
            raise ValueError(f"encode_chunk takes [B = {B}, n, F] feature frames, n a positive multiple of {factor}")
        host, nv = _frame_counts(m, feats, nframes)
        x = feats.contiguous()
        rows = x.shape[1]
        for mod, tail in zip(m.modules["convs"], self.conv_tails):
            w, bias, scale, shift = m._conv_consts(mod["name"])
            shape = (mod["kh"], mod["kw"], mod["cin"], mod["cout"])
            lead = 0 if tail is None else tail.shape[1]
            win = x.view(B, rows, -1) if tail is None else torch.cat([tail, x.view(B, rows, -1)], 1)
            x = K.conv2d_fwd(win.view(B, lead + rows, -1, mod["cin"]), w, shape, bias=bias, scale=scale, shift=shift, relu=True,
                             strides=(mod["st"], mod["sf"]), padding="causal", lead=lead)
            if tail is not None:
                K.conv1d_tail_update(win, nv, tail)
            if mod["st"] > 1:
                nv = ((nv + (mod["st"] - 1)) // mod["st"]).to(torch.int32).contiguous()
            rows = x.shape[1]
        x = x.view(B, rows, -1)
        for li, r in enumerate(m.modules["rnns"]):
            k, b, rk = m._rnn_consts(r)
            P = r["P"]
            y = self.lstm.run(li, K.matmul(x.view(B * rows, x.shape[2]), k, bias=b).view(B, rows, 4 * P), rk, nv)
            if r["rowconv"]:
                scale, shift = m._affine(r["rowconv"] + "/bn")
                y = K.stream_rowconv_fwd(y.view(B * rows, P), self.row_tails[li], m.ps.p(r["rowconv"] + "/conv/w"), scale, shift, nv, B, rows)
            x = y.view(B, rows, P)
        for f in m.modules["fcs"]:
            w, bias = m._fc_consts(f)
            x = K.conv1d_fwd(x, w, (1, f["din"], f["dout"]), bias=bias, relu=True)
        return x.view(B, rows, c.dmodel), nv, self._reduced(host)


def _out_rows(fb, n):
    """rows of the output buffer of a step of n feature frames through the boundary reductions fb (the most frames one step can complete)"""
    for f in fb:
        n = -(-(f - 1 + n) // f) if f > 1 else n
    return n


class RnntStreamState(EncoderStream):
    """Encoder state of `batch_size` streams of the RNN-Transducer encoder (forward LSTMs and row-wise layers only: every config streams
    exactly).  Per stream:
        each block       h and c [rnn_units] f32 (_CarriedLstm)
        each reduction   the rows that do not fill a group yet, [factor - 1, width] in the compute type, and their count: INPUT rows in
                         front of a `pre` reduction, PROJECTED rows behind a `post` one
    The reductions are kept per block BOUNDARY (rnnt.boundary_factors): boundary 0 is block 0's `pre` reduction, boundary i
    block i - 1's `post` times block i's `pre` (a reduction by f followed by one by g groups f g consecutive rows - zero rows pad either,
    and no layer sits between them), the last one the last block's `post`.  The counts live on the host (`cnt`, the step's launch
    arguments are computed from them) and ride in export / load as one int32 tensor [boundaries, B] behind the carried tensors."""
    uses_final = True
    host_tensors = 1

    def __init__(self, model, batch_size):
        super().__init__(model, batch_size)
        B, dev, dt, mods = self.B, model.device, model.dtype, model.modules
        self.fb = model.boundary_factors()
        widths = [int(model.cfg.num_feature_bins)] + [m["dout"] for m in mods]
        self.lstm = _CarriedLstm(model, B, [m["P"] for m in mods])
        self.carry = [torch.zeros(B, f - 1, w, dtype=dt, device=dev) if f > 1 else None for f, w in zip(self.fb, widths)]
        self.cnt = [[0] * B for _ in self.fb]
        self.last_nvalid = [0] * B  # encoder frames the last step gave each stream (host)

    @staticmethod
    def step_rule(cfg, chunk_frames=None):
        """a step is `chunk_frames` feature frames, any positive number: what does not fill a reduction's group is carried, so the encoder
        frames a step gives depend on the state (encode's host list), out_rows(chunk_frames) at the most"""
        n = int(chunk_frames if chunk_frames is not None else 32)
        if n < 1:
            raise ValueError(f"stream: chunk_frames {n} must be positive")
        return n, _out_rows(boundary_factors(rnnt_modules(cfg)), n), cfg.encoder_length

    def _tensors(self):
        return self.lstm.tensors() + [t for t in self.carry if t is not None]

    def _host_reset(self, rows):
        for c in self.cnt:
            for b in rows:
                c[b] = 0

    def _host_export(self):
        return [torch.tensor(self.cnt, dtype=torch.int32, device=self.model.device)]

    def _host_load(self, tensors):
        cnt = tensors[0].cpu().tolist()
        if len(cnt) != len(self.fb) or any(len(r) != self.B or min(r) < 0 or max(r) >= max(f, 1) for r, f in zip(cnt, self.fb)):
            raise ValueError("encoder state of another model")
        self.cnt = [[int(v) for v in r] for r in cnt]

    def reference_states(self):
        return self.lstm.reference_states()

    def out_rows(self, n):
        """rows of the step's output buffer for n feature frames (the most frames one step can complete)"""
        return _out_rows(self.fb, n)

    @torch.no_grad()
    def encode(self, feats, nframes, final=()):
        """One encoder step of the RNN-Transducer: feats [B, n, F] (compute type, device), nframes [B] feature frames that are real per
        stream (0 = idle .. n), final = the streams whose utterance ends with these frames -> (enc [B, out_rows(n), cfg.dmodel], nvalid [B]
        int32 device, nvalid on the host = last_nvalid); advances state.  Every stream advances by its own number of frames: in front of
        each reduction its carried rows and its new rows form groups, whole groups go on, the rest is carried; a final stream's last group
        is filled with zero rows, as tf.pad fills it offline.  Per block: one GEMM, the recurrence continued from the carried state
        (_CarriedLstm.run, lengths = the stream's groups), and tfasr_rnnt_block_tail_fwd writing each stream's rows behind the rows the next
        reduction carries (`off`).  A boundary no tail kernel writes - block 0's `pre` reduction, the two-launch tail - is assembled by a
        gather instead."""
        m = self.model
        c, B, mods, fb = m.cfg, self.B, m.modules, self.fb
        if feats.dim() != 3 or feats.shape[0] != B or feats.shape[1] < 1:
            raise ValueError(f"encode_chunk takes [B = {B}, n >= 1, F] feature frames")
        host, _ = _frame_counts(m, feats, nframes, upload=False)
        fin = [False] * B
        for b in final:
            fin[int(b)] = True
        # everything the launches need is known on the host: per boundary the carried count (the tail's `off`), the rows that enter (to zero
        # a final stream's padding), the groups that go on (the block's lengths) and where the new carry starts
        L = len(mods)
        plan, come = [], host
        for i, f in enumerate(fb):
            cnt = self.cnt[i] if f > 1 else [0] * B
            avail = [a + b for a, b in zip(cnt, come)]
            groups = [(-(-a // f) if fin[b] else a // f) for b, a in enumerate(avail)]
            plan.append(dict(cnt=list(cnt), avail=avail, groups=groups, start=[g * f for g in groups]))
            if f > 1:
                self.cnt[i] = [0 if fin[b] else a - g * f for b, (a, g) in enumerate(zip(avail, groups))]
            come = groups
        vec = m._h2d(np.asarray([p[k] for p in plan for k in ("cnt", "groups", "start")], np.int32))
        dv = lambda i, k: vec[3 * i + ("cnt", "groups", "start").index(k)]

        def reduce(i, x):
            """boundary i over x [B, R, w] (R % f == 0, each stream's carried rows in front): -> [B, R / f, f w]; moves the carry"""
            f = fb[i]
            if f == 1:
                return x
            R, w = x.shape[1], x.shape[2]
            for b in range(B):  # tf.pad's zero rows of a last, partial group
                lo, hi = plan[i]["avail"][b], plan[i]["start"][b]
                if fin[b] and hi > lo:
                    x[b, lo:hi].zero_()
            K.conv1d_tail_update(x, dv(i, "start"), self.carry[i])
            return x.view(B, R // f, f * w)

        x = feats.contiguous()
        if fb[0] > 1:
            x = _place(self.carry[0], dv(0, "cnt"), x, -(-(fb[0] - 1 + x.shape[1]) // fb[0]) * fb[0])
        for i, mod in enumerate(mods):
            x = reduce(i, x)
            T, P, N = x.shape[1], mod["P"], mod["dout"]
            lens = dv(i, "groups")
            ps, p = m.ps, mod["name"] + "/lstm"
            xg = K.matmul(x.reshape(B * T, x.shape[2]), ps.w2d(p + "/k"), bias=ps.p(p + "/b")).view(B, T, 4 * P)
            y = self.lstm.run(i, xg, ps.w(p + "/rk").view(1, P, 4 * P), lens)
            f = fb[i + 1]
            Tpad = -(-(f - 1 + T) // f) * f if f > 1 else T
            if m._fused_tail(mod):
                out = torch.empty(B, Tpad, N, dtype=y.dtype, device=y.device)
                if f > 1:
                    out[:, :f - 1].copy_(self.carry[i + 1])
                x, _ = m.tail_fwd(y, mod, lens, Tpad, 1, off=dv(i + 1, "cnt") if f > 1 else None, out=out)
            else:
                x, _ = m.tail_fwd(y, mod, lens, T, 1)
                if f > 1:
                    x = _place(self.carry[i + 1], dv(i + 1, "cnt"), x, Tpad)
        x = reduce(L, x)
        self.last_nvalid = plan[L]["groups"]
        return x.reshape(B, x.shape[1], c.dmodel), dv(L, "groups"), list(self.last_nvalid)


def _place(carry, cnt_dev, new, R):
    """[carry rows 0 .. cnt - 1 | new rows] per stream as one [B, R, w] buffer (rows past cnt + new.shape[1] repeat the last row: callers
    never read them, or zero them).  The ragged copy of a boundary no tail kernel writes: block 0's input, and the two-launch tail."""
    B, n, w = new.shape
    cat = torch.cat([carry, new], 1)
    r = torch.arange(R, device=new.device)[None, :]
    c = cnt_dev.long()[:, None]
    idx = torch.where(r < c, r, r - c + carry.shape[1]).clamp_(max=cat.shape[1] - 1)
    return torch.gather(cat, 1, idx[:, :, None].expand(B, R, w))


STREAM_STATES = {"conformer": StreamState, "transformer": TransformerStreamState, "jasper": JasperStreamState, "deepspeech2": DS2StreamState,
                 "rnnt": RnntStreamState}


def check_streamable(model):
    """-> the state class of the model's encoder (STREAM_STATES), after that class's refusal rule"""
    cls = STREAM_STATES.get(getattr(model.cfg, "encoder", "conformer"))
    if cls is None:
        raise ValueError("streaming needs a Conformer encoder: ContextNet's squeeze-and-excite is a mean over the whole utterance")
    cls.check(model)
    return cls


def _twin(model, precision):
    return model.inference_twin() if (precision or model.decode_precision) == "f32" else model


def encode_chunk(state, feats, nframes, final=()):
    """One encoder step of any state (its `encode`, without the host list): -> (enc, nvalid [B] int32 device); advances state."""
    return state.encode(feats, nframes, final)[:2]


transformer_encode_chunk = jasper_encode_chunk = ds2_encode_chunk = rnnt_encode_chunk = encode_chunk


def check_stream_args(batch_size=1, max_tokens_per_frame=3, beam_width=0, max_frames=3000):
    """The session arguments that need no device to judge -> them as ints.  beam_width 0 = the greedy session; 1 .. 64 = a beam of that
    many hypotheses per stream (the device searches keep a beam in one workgroup's LDS: 64 rows at most)."""
    batch_size, max_tokens_per_frame, beam_width, max_frames = int(batch_size), int(max_tokens_per_frame), int(beam_width), int(max_frames)
    if batch_size < 1:
        raise ValueError(f"stream: batch_size {batch_size} must be >= 1")
    if max_tokens_per_frame < 1:
        raise ValueError(f"stream: max_tokens_per_frame {max_tokens_per_frame} must be >= 1")
    if not 0 <= beam_width <= 64:
        raise ValueError(f"stream: beam_width {beam_width} outside [0, 64] (0 = greedy; a beam lives in one workgroup's LDS)")
    if max_frames < 1:
        raise ValueError(f"stream: max_frames {max_frames} must be >= 1 (the encoder frames one stream may consume between resets)")
    return batch_size, max_tokens_per_frame, beam_width, max_frames


def check_commit_horizon(commit_horizon, beam_width):
    """commit_horizon (None = no horizon) against the session's beam_width -> None or the horizon in encoder frames"""
    if commit_horizon is None:
        return None
    if int(beam_width) < 1:
        raise ValueError("stream: commit_horizon belongs to a beam session (beam_width >= 1): the greedy searches commit every token at once")
    h = int(commit_horizon)
    if not 1 <= h <= K.MAX_HORIZON:
        raise ValueError(f"stream: commit_horizon {h} outside [1, {K.MAX_HORIZON}] encoder frames")
    return h


def check_stream_lm(model, lm, lm_alpha, lm_beta, beam_width, detail=False):
    """A session's n-gram LM (None = none) against the model and the session, before any device work -> None, or the tables
    NGramLM.tables(lm_alpha, lm_beta) the fused beam runs on."""
    if lm is None:
        return None
    if model.cfg.head != "ctc":
        raise NotImplementedError(f"{type(model).__name__}.stream(lm=...): LM shallow fusion exists for the CTC prefix beam search only; a "
                                  "transducer's prediction network is its LM")
    if detail:
        raise ValueError("stream: lm belongs to a beam session; detail sessions are greedy")
    if int(beam_width) < 1:
        raise ValueError("stream: lm belongs to a beam session (beam_width >= 1): the greedy search takes one class per frame and has no "
                         "hypotheses for a language model to rank")
    if int(beam_width) > K.CTC_LM_MAX_BEAM:
        raise ValueError(f"stream: beam_width {int(beam_width)} with lm is outside [1, {K.CTC_LM_MAX_BEAM}] (the fused candidate list of a "
                         "frame lives in one workgroup's LDS)")
    model._check_lm(lm)
    return lm.tables(lm_alpha, lm_beta)


class _TokenRecord:
    """The tokens of one stream of a detail session since its reset, on the host: class, frame (CTC: the first frame of the run), end (CTC:
    one past the run's last frame, -1 while the run is open; transducer: frame + 1), log-probability, entropy."""

    def __init__(self):
        self.tokens, self.frames, self.ends, self.logp, self.ent = [], [], [], [], []

    def extend(self, tokens, frames, ends, logp, ent):
        self.tokens += tokens
        self.frames += frames
        self.ends += [f + 1 for f in frames] if ends is None else ends
        self.logp += logp
        self.ent += ent

    def update_last(self, end, logp, ent):
        """the CTC token that was open went on, or closed"""
        self.ends[-1], self.logp[-1], self.ent[-1] = end, logp, ent

    @property
    def open(self):
        return bool(self.ends) and self.ends[-1] < 0


class StreamingRecognizer:
    """model.stream(): accept() PCM as it arrives, get the new tokens back; finish() flushes a stream's tail.

    beam_width = 0: the greedy search (recognize_single's rule, up to max_tokens_per_frame symbols per frame).
    beam_width >= 1: the device beam search (at most ONE symbol per frame) with the whole beam carried from chunk to chunk: after any
    sequence of accept calls stream b holds exactly the beam recognize_beam_encoded / recognize_nbest hold after the same encoder frames
    (f32 on the f32 master weights whatever the encoder's type).  StreamOutput.tokens are then the tokens COMMITTED by the call: the
    labels new in the prefix that every live hypothesis shares, which can no longer change; finish() commits the rest of the best
    hypothesis, so the concatenation of a stream's outputs is its best path.  hypotheses() gives the current n-best in full.  Because the
    beam emits one symbol per frame at most, a beam_width=1 session equals the greedy session made with max_tokens_per_frame=1, not the
    default greedy session.  The CTC head's beam session treats class V-1 as blank, as recognize_beam does.
    model.stream_lm(lm, ..., lm_alpha=0.5, lm_beta=0.0) (then stream()'s arguments; the stream() signatures are pinned and stay as they
    are), model.stream_horizon(H, ..., lm=lm, lm_alpha=, lm_beta=) or rec.with_lm(lm, lm_alpha, lm_beta) before the first accept, with
    lm = an lm.NGramLM (CTC heads, 1 <= beam_width <= 32; lm_alpha, lm_beta as recognize_beam_lm's alpha, beta): the beam is the fused
    search's (K.CtcLmBeamStream on lm.tables(lm_alpha, lm_beta)), stream b holds the beam recognize_nbest_lm holds after
    the same encoder frames, and the blank is the model's OWN, self.blank, as recognize_beam_lm uses - NOT the V-1 convention of the
    plain beam session above.  Commits follow the LM-ranked best row; a running stream ranks without the end-of-sentence term, a
    finished one with it.  hypotheses() keeps its three values (scores = the fused score), hypotheses_lm() adds log_prob and lm_score.
    lm with beam_width 0, beam_width > 32 or a detail session is a ValueError, with a transducer head NotImplementedError.
    max_frames bounds the encoder frames of one stream between resets (a chunk past it raises RuntimeError; reset() frees the slot).

    commit_horizon = H (beam sessions) makes the session endless and its committed text prompt, at a price in accuracy: a
    label that the best hypothesis has held for H encoder frames is final, and the hypotheses that disagree with it leave the beam.  It
    is a pruning rule: the result can differ from the offline search's.  The commit then runs after EVERY chunk (the prune points are the
    chunk boundaries, which the config fixes: the tokens do not depend on how the samples arrive), a call returns its chunks' commits
    in a row, and max_frames bounds only the UNCOMMITTED part of a stream: before a chunk that would take a stream's trie past it the
    session compacts that stream (K.*BeamStream.compact: everything above and beside the live hypotheses goes; compact() does it on
    demand), keeps the dropped labels on the host, and goes on.  Only when the stream still does not fit - its uncommitted part alone is
    too long - the chunk raises RuntimeError, naming the stream and the lengths.  That is decided chunk by chunk, not before the call as
    without a horizon: the chunks before the refused one have been consumed and searched, their commits are in committed_tokens and in
    hypotheses(); the refused chunk's samples and all later ones stay buffered (for an RNN-Transducer encoder, whose frames per step
    depend on carried rows, a refusal can also come after the step's encoder pass, which has then consumed its samples); reset(rows=[b])
    frees the slot.  hypotheses() returns full hypotheses (committed prefix + what the trie holds), StreamOutput.frames counts from the
    stream's reset.  Open it with model.stream_horizon(H, ...) (then stream()'s arguments), or with commit_horizon=H here.
    Beam memory per stream, with W = beam_width, N = 1 + W * max_frames trie nodes and H = the power of two >= 2 N table slots:
        transducer  12 N + 12 H + W * (4 V + 44 U + 8 J + 12 min(2 W, V - 1) + 28) bytes   (U = rnn_units, J = joint_dim)
        CTC         12 N + 12 H + 24 W + 8 chunk_size * (1 + min(2 W, V - 1)) bytes
    (W = 10, max_frames = 3000, V = 1000, U = J = 320: about 1.4 MB per stream.)

    A Jasper model (causal convolutions only) opens the same session through JasperCTC.stream(batch_size, chunk_frames=...): a step is
    chunk_frames feature frames instead of 4 * chunk_size, its encoder state is JasperStreamState (per layer with K > 1 taps the last
    (K - 1) * dilation input rows, sum over layers of B * (K - 1) * dilation * Cin elements), and in the CTC beam formula above chunk_size
    reads chunk_frames / time_reduction_factor.  The unidirectional DeepSpeech2 opens it the same way (DeepSpeech2CTC.stream); its encoder
    state is DS2StreamState.

    A Transformer model with a chunked config (TransformerCTC.stream / TransformerTransducer.stream) takes the Conformer's step,
    4 * chunk_size feature frames, and the Conformer's frame reduction; its encoder state is TransformerStreamState (per block two rings of
    B * history_size * num_heads * head_size elements, plus the two subsampling carries).

    An RNN-Transducer (RnnTransducer.stream(batch_size, chunk_frames=...)) takes steps of any positive number of feature frames: its
    encoder state is RnntStreamState (per block the LSTM's h and c, per time reduction the rows that do not fill a group yet), the encoder
    frames a step gives depend on those carried rows, and finish() sends a final step that zero-pads each reduction's last group - a step
    without feature frames when the utterance ended on a step boundary.

    A detail session (model.stream_detailed(...) with stream()'s arguments, or detail=True here; greedy only): accept / finish return a StreamDetailOutput - the same tokens, plus the frame, the
    log-probability and the entropy of each, frames counted from the stream's reset - and the session keeps every stream's record:
    recognized() is what recognize_detailed gives the utterance so far, open_tokens() the CTC streams whose last token's run may still
    go on, trailing_blank_frames() the frames since the last token.  The transducer's search runs the detail variants of the same mode-2
    launches; the CTC head runs tfasr_ctc_greedy_decode_carry_detail (one launch) on a carried K.CtcDetailState, and finish() closes an
    open run with the final flag."""

    def __init__(self, model, batch_size=1, precision=None, max_tokens_per_frame=3, beam_width=0, max_frames=3000, chunk_frames=None,
                 commit_horizon=None, detail=False):
        batch_size, max_tokens_per_frame, self.beam_width, self.max_frames = check_stream_args(batch_size, max_tokens_per_frame, beam_width,
                                                                                             max_frames)
        self.commit_horizon = check_commit_horizon(commit_horizon, self.beam_width)
        self.lm_tables = None  # with_lm(): the tables of the session's n-gram LM
        self.detail = self._check_detail(detail)
        self.model = model
        self.enc_model = _twin(model, precision)
        self.B = int(batch_size)
        self.max_tokens_per_frame = int(max_tokens_per_frame)
        c = model.cfg
        # everything the session knows about the encoder is its state class (EncoderStream): the refusal rule, the step rule, the state
        cls = check_streamable(self.enc_model)
        self.chunk_frames, self.C, self._reduce = cls.step_rule(c, chunk_frames)
        self.state = cls(self.enc_model, batch_size)
        self.step, self.flen = int(c.frame_step), int(c.frame_length)
        self.chunk_samples = self.step * (self.chunk_frames - 1) + self.flen  # samples a full chunk's feature frames cover
        self.ctc = c.head == "ctc"
        self.encoded_log = None  # a list here receives (enc [B, C, d], nvalid host list) of every chunk (callers that want the frames)
        self.chunks_run = 0
        self._init_rows(range(self.B), first=True)

    # ------------------------------------------------------------------------------------------- state
    def _init_rows(self, rows, first=False):
        m, dev, B = self.model, self.model.device, self.B
        if first:
            self.buf = [np.zeros(0, np.float32) for _ in range(B)]
            self.prev = np.zeros(B, np.float32)
            self.has_prev = np.zeros(B, np.int32)
            self.total = [0] * B  # samples received
            self.emitted = [0] * B  # feature frames consumed
            self.frames = [0] * B  # encoder frames emitted
            self.finished = [False] * B
            self.flushed = [False] * B  # (state.uses_final) the encoder's carried rows went out with a final step
            self.beam = None
            self.committed_tokens = [[] for _ in range(B)]  # (horizon sessions) everything a stream has committed since its reset
            if self.detail:  # the record of every stream since its reset: what recognized() returns
                self.record = [_TokenRecord() for _ in range(B)]
            if self.beam_width:
                self.beam = self._new_beam()
            elif self.ctc and self.detail:
                self.ctc_state = K.CtcDetailState(B, dev)
            elif self.ctc:
                self.last_class = torch.full((B,), -1, dtype=torch.int32, device=dev)
            else:
                P = m.cfg.rnn_units
                self.prev_tok = torch.full((B,), m.blank, dtype=torch.int32, device=dev)
                self.h = torch.zeros(B, P, dtype=torch.float32, device=dev)
                self.c = torch.zeros(B, P, dtype=torch.float32, device=dev)
                self._packed = None
            return
        rows = list(rows)
        for b in rows:
            self.buf[b] = np.zeros(0, np.float32)
            self.prev[b], self.has_prev[b] = 0.0, 0
            self.total[b] = self.emitted[b] = self.frames[b] = 0
            self.finished[b] = self.flushed[b] = False
            self.committed_tokens[b] = []
        r = torch.as_tensor(rows, dtype=torch.long, device=dev)
        if self.detail:
            for b in rows:
                self.record[b] = _TokenRecord()
        if self.beam is not None:
            self.beam.reset(rows)
        elif self.ctc and self.detail:
            self.ctc_state.reset(rows)
        elif self.ctc:
            self.last_class[r] = -1
        else:
            self.prev_tok[r] = m.blank
            self.h[r] = 0
            self.c[r] = 0

    def reset(self, rows=None):
        """Zero the state of some or all streams: the slot takes the next utterance."""
        rows = list(range(self.B)) if rows is None else list(rows)
        self.state.reset(None if len(rows) == self.B else rows)
        self._init_rows(rows)

    def encoder_state(self):
        return self.state.export()

    def set_encoder_state(self, tensors):
        self.state.load(tensors)

    # ------------------------------------------------------------------------------------------- steps
    def _take(self, n, total, emitted, flush):
        """the chunk-taking rule: the feature frames a stream gives the next step from n buffered samples - a full chunk, or under `flush`
        what its `total` samples still hold behind the `emitted` frames"""
        if n >= self.chunk_samples:
            return self.chunk_frames
        return min(-(-total // self.step) - emitted, self.chunk_frames) if flush else 0

    def _ready(self, b, flush):
        """feature frames stream b can give to the next chunk"""
        return self._take(len(self.buf[b]), self.total[b], self.emitted[b], flush and not self.finished[b])

    @torch.no_grad()
    def _run(self, flush_rows=()):
        m, em, dev, B, st = self.model, self.enc_model, self.model.device, self.B, self.state
        c = m.cfg
        new = [[] for _ in range(B)]
        mark = [len(r.tokens) for r in self.record] if self.detail else None  # where this call's tokens begin in the record
        window, melw, band = em._frontend_consts()
        while True:
            take = [self._ready(b, b in flush_rows) for b in range(B)]
            final = ()
            if st.uses_final:  # the streams whose utterance ends with this step: their carried rows go out, the last group zero-padded
                final = [b for b in flush_rows if not self.finished[b] and not self.flushed[b]
                         and -(-self.total[b] // self.step) - self.emitted[b] - take[b] == 0]
            if max(take) == 0 and not final:
                break
            # one front-end launch per chunk on exactly the samples the chunk's frames cover: the same frames whatever the arrival
            sig = np.zeros((B, self.chunk_samples), np.float32)
            nlen = np.zeros(B, np.int32)
            for b in range(B):
                if take[b]:
                    seg = self.buf[b][:self.chunk_samples]
                    sig[b, :len(seg)] = seg
                    nlen[b] = len(seg)
            if max(take) == 0:  # (a final step) nothing but carried encoder rows is left to flush: no frame is read
                feats = torch.zeros(B, self.chunk_frames, c.num_feature_bins, dtype=em.dtype, device=dev)
            else:
                feats = K.logmel_stream(em._h2d(torch.from_numpy(sig), torch.float32), em._h2d(nlen), em._h2d(torch.from_numpy(self.prev.copy()), torch.float32),
                                        em._h2d(self.has_prev.copy()), self.chunk_frames, window, melw, band, c.frame_step, c.nfft, c.preemphasis,
                                        c.epsilon, torch.float32 if st.f32_features else em.dtype)
                feats = st.prepare(feats)
            if self.commit_horizon:
                self._make_room([self._reduce(t) if t else 0 for t in take])  # before anything of the chunk is consumed
            for b in range(B):
                if take[b]:
                    used = take[b] * self.step
                    if used <= len(self.buf[b]):
                        self.prev[b], self.has_prev[b] = self.buf[b][used - 1], 1
                    self.buf[b] = self.buf[b][used:]
                    self.emitted[b] += take[b]
            enc, nvalid, nv = st.encode(feats, take, final)
            for b in final:
                self.flushed[b] = True
            if self.encoded_log is not None:
                self.encoded_log.append((enc, nv))
            self.chunks_run += 1
            if self.beam is not None:
                if self.commit_horizon:
                    self._make_room(nv)  # (exact now; differs from the estimate only for encoders with carried rows)
                self._advance_beam(enc, nv)
                if self.commit_horizon:
                    self._take_commit(new, self.beam.commit(horizon=self.commit_horizon))
            else:
                toks = self._search_ctc(enc, nvalid) if self.ctc else self._search(enc, nvalid, nv)
            for b in range(B):
                self.frames[b] += nv[b]
                if self.beam is None:
                    new[b].extend(toks[b])
        if self.commit_horizon:  # every chunk has committed; the flushed streams commit the rest of their best row
            if flush_rows:
                self._take_commit(new, self.beam.commit(final_rows=sorted(flush_rows), horizon=self.commit_horizon))
        elif self.beam is not None:  # one commit per call: the labels that became stable, and the rest of the best row for flushed streams
            self._take_commit(new, self.beam.commit(final_rows=sorted(flush_rows)))
        if self.detail and self.ctc:
            closing = [b for b in flush_rows if not self.finished[b] and self.record[b].open]
            if closing:  # the utterance is over: close the run that reached its last frame (a call without frames, the final flag alone)
                self._ctc_detail(torch.zeros(B, 1, c.vocab_size, dtype=torch.float32, device=dev), em._h2d([0] * B),
                                 em._h2d([int(b in closing) for b in range(B)]))
        W = max(max(len(t) for t in new), 1)
        out = torch.full((B, W), m.blank, dtype=torch.int32)
        for b in range(B):
            if new[b]:
                out[b, :len(new[b])] = torch.tensor(new[b], dtype=torch.int32)
        plain = StreamOutput(out, torch.tensor([len(t) for t in new], dtype=torch.int32), torch.tensor(self.frames, dtype=torch.int32))
        if not self.detail:
            return plain
        assert all(r.tokens[k:] == t for r, k, t in zip(self.record, mark, new))  # the record's new part is the call's tokens
        pad = lambda rows, fill, dtype: torch.tensor([row[k:] + [fill] * (W - len(row) + k) for row, k in zip(rows, mark)], dtype=dtype)
        rec = self.record
        return StreamDetailOutput(*plain, pad([r.frames for r in rec], -1, torch.int32),
                                  pad([r.ends for r in rec], -1, torch.int32) if self.ctc else None,
                                  pad([r.logp for r in rec], 0.0, torch.float32), pad([r.ent for r in rec], 0.0, torch.float32))

    # ------------------------------------------------------------------------------------------- beam sessions
    def _new_beam(self):
        m = self.model
        ps, c = m.ps, m.cfg
        if self.ctc and self.lm_tables is not None:
            return K.CtcLmBeamStream(self.B, self.C, self.max_frames, c.vocab_size, self.beam_width, self.lm_tables, blank_index=m.blank,
                                     device=m.device)
        if self.ctc:
            return K.CtcBeamStream(self.B, self.C, self.max_frames, c.vocab_size, self.beam_width, blank_index=None, device=m.device)
        lng, lnb = (ps.p("pred/ln/g"), ps.p("pred/ln/b")) if c.prediction_layer_norm else (None, None)
        weights = (ps.p("pred/emb"), ps.p2d("pred/lstm/k"), ps.p2d("pred/lstm/rk"), ps.p("pred/lstm/b"), lng, lnb, ps.p2d("joint/pred/w"),
                   ps.p("joint/pred/b"), ps.p2d("joint/vocab/w"), ps.p("joint/vocab/b"))
        return K.RnntBeamStream(weights, self.B, self.max_frames, self.beam_width, blank=m.blank)

    def _take_commit(self, new, commit):
        """a commit's (tokens, counts) -> appended to the call's tokens and to the streams' committed tokens"""
        th, tl = commit[0].cpu(), commit[1].cpu()
        for b in range(self.B):
            t = th[b, :int(tl[b])].tolist()
            new[b] += t
            self.committed_tokens[b] += t

    def _make_room(self, need):
        """(horizon sessions) need[b] more frames for stream b's trie: compact the streams they would take past max_frames; refuse when
        one still does not fit"""
        over = [b for b in range(self.B) if self.beam.frames[b] + need[b] > self.max_frames]
        if not over:
            return
        self.beam.compact(over)
        for b in over:
            if self.beam.frames[b] + need[b] > self.max_frames:
                raise RuntimeError(f"stream {b}: its uncommitted hypotheses alone are {self.beam.frames[b]} labels deep after {self.frames[b]} "
                                   f"frames ({len(self.beam.dropped[b])} labels committed and dropped) and the next chunk adds {need[b]} frames, past "
                                   f"max_frames = {self.max_frames}: reset it, or open the session with a larger max_frames or a shorter "
                                   "commit_horizon")

    def compact(self, rows=None):
        """Compact the beam tries of the given streams (default: all) now -> per stream [labels dropped, trie nodes kept, trie frames]
        (K.*BeamStream.compact).  A horizon session does it by itself when a stream reaches max_frames."""
        if self.beam is None:
            raise ValueError("compact() needs a beam session: open it with model.stream(beam_width >= 1)")
        return self.beam.compact(rows)

    def with_lm(self, lm, lm_alpha=0.5, lm_beta=0.0):
        """This beam session, which has taken no audio yet, with the n-gram model `lm` fused into its carried beam (what model.stream_lm
        returns; lm=None: the session as it is) -> self.  The beam becomes a K.CtcLmBeamStream on lm.tables(lm_alpha, lm_beta) and the
        model's own blank.  Refused with the reason: a transducer head (NotImplementedError); a greedy or detail session, beam_width >
        32, an lm of another vocabulary (ValueError)."""
        if lm is None:
            return self
        if any(self.total) or self.chunks_run:
            raise RuntimeError("stream: with_lm() comes before the first accept()")
        self.lm_tables = check_stream_lm(self.model, lm, lm_alpha, lm_beta, self.beam_width, self.detail)
        self.beam = self._new_beam()
        return self

    def with_commit_horizon(self, commit_horizon):
        """This session, which has taken no audio yet, as a horizon session (what model.stream_horizon returns) -> self."""
        if any(self.total) or self.chunks_run:
            raise RuntimeError("stream: with_commit_horizon() comes before the first accept()")
        if self.detail:
            raise ValueError("stream: commit_horizon belongs to a beam session; detail sessions are greedy")
        self.commit_horizon = check_commit_horizon(commit_horizon, self.beam_width)
        return self

    def _check_capacity(self, flush_rows=(), more=None):
        """refuse a call (more[b] further samples, or the flush of some streams) whose chunks would take a stream past max_frames, before
        anything of it is buffered or queued: the session stays as it was.  (A horizon session compacts as it goes and decides chunk by
        chunk: _make_room.)"""
        if self.beam is None or self.commit_horizon:
            return
        for b in range(self.B):
            n, emitted, frames = len(self.buf[b]) + (more[b] if more else 0), self.emitted[b], self.frames[b]
            total = self.total[b] + (more[b] if more else 0)
            flush = b in flush_rows and not self.finished[b]
            while True:  # the chunks _run will take from this stream
                take = self._take(n, total, emitted, flush)
                if take <= 0:
                    break
                n, emitted, frames = max(n - take * self.step, 0), emitted + take, frames + self._reduce(take)
            if self.state.uses_final:  # a step's frames depend on the carried rows; all steps together never give more than the utterance so far
                frames = self._reduce(emitted)
            if frames > self.max_frames:
                raise RuntimeError(f"stream {b} would pass max_frames = {self.max_frames} encoder frames ({self.frames[b]} so far, {frames} after "
                                   "this call): reset it, or open the session with a larger max_frames")

    def _advance_beam(self, enc, nv):
        m = self.model
        ps = m.ps
        B, C, _ = enc.shape
        if self.ctc:
            logits = K.matmul(self._enc32(enc), ps.p2d("dec/logits/w"), bias=ps.p("dec/logits/b")).view(B, C, m.cfg.vocab_size)
            self.beam.advance(logits, nv)
        else:
            encj = K.matmul(self._enc32(enc), ps.p2d("joint/enc/w"), bias=ps.p("joint/enc/b")).view(B, C, m.cfg.joint_dim)
            self.beam.advance(encj, nv)

    def hypotheses(self, top_paths=None):
        """The current n-best of every stream in full, committed part included: (tokens [B, P, L] blank padded (CTC: 0 padded), lengths
        [B, P], scores [B, P]) device tensors, best first; P = top_paths (default: beam_width).  Valid after every accept and after
        finish, until reset."""
        return self._hypotheses(top_paths)[:3]

    def hypotheses_lm(self, top_paths=None):
        """hypotheses() of a session opened with lm=...: (tokens, lengths, score, log_prob, lm_score), as recognize_nbest_lm returns them.
        The streams that have been finished rank with the end-of-sentence term (lm_score includes it); running ones rank by log_prob +
        lm, without it."""
        if self.lm_tables is None:
            raise ValueError("hypotheses_lm() needs a beam session with a language model: open it with model.stream(beam_width >= 1, lm=...)")
        return self._hypotheses(top_paths)

    def _hypotheses(self, top_paths):
        if self.beam is None:
            raise ValueError("hypotheses() needs a beam session: open it with model.stream(beam_width >= 1)")
        if self.lm_tables is not None:
            toks, lens, scores, *rest = self.beam.nbest(top_paths, final_rows=[b for b in range(self.B) if self.finished[b]])
        else:
            (toks, lens, scores), rest = self.beam.nbest(top_paths)[:3], []
        dropped = self.beam.dropped
        if not any(dropped):
            return (toks, lens, scores, *rest)
        # compacted streams: the labels their tries dropped go back in front of every live row
        th, lh, live = toks.cpu(), lens.cpu(), (scores != -float("inf")).cpu()
        P = th.shape[1]
        full = torch.full((self.B, P, max(max(self.frames), 1)), 0 if self.ctc else self.model.blank, dtype=torch.int32)
        for b in range(self.B):
            d = torch.tensor(dropped[b], dtype=torch.int32)
            for p in range(P):
                if live[b, p]:
                    n = int(lh[b, p])
                    full[b, p, :len(d)] = d
                    full[b, p, len(d):len(d) + n] = th[b, p, :n]
                    lh[b, p] = len(d) + n
        return (full.to(toks.device), lh.to(lens.device), scores, *rest)

    def _enc32(self, enc):
        B, C, d = enc.shape
        e = enc.reshape(B * C, d)
        if e.dtype != torch.float32:
            e = K.cast(e.contiguous(), torch.empty(B * C, d, dtype=torch.float32, device=e.device))
        return e

    def _search(self, enc, nvalid, nv_host):
        """The greedy search of recognize_single continued over this chunk for every stream on its own (mode 2 of csrc/decode.hip)."""
        m = self.model
        ps, c, dev = m.ps, m.cfg, m.device
        B, C, _ = enc.shape
        P, J, V = c.rnn_units, c.joint_dim, c.vocab_size
        f32 = torch.float32
        encj = K.matmul(self._enc32(enc), ps.p2d("joint/enc/w"), bias=ps.p("joint/enc/b")).view(B, C, J)
        mtpf = self.max_tokens_per_frame
        max_tokens = C * mtpf
        if self.detail:  # tokens + frames and log-probabilities + entropies in two buffers (two fetches, not four), pre-filled blank / -1 / 0 / 0
            ibuf = torch.full((2, B, max_tokens), -1, dtype=torch.int32, device=dev)
            ibuf[0] = m.blank
            fbuf = torch.zeros(2, B, max_tokens, dtype=f32, device=dev)
            tokens, detail = ibuf[0], (ibuf[1], fbuf[0], fbuf[1])
        else:
            tokens = torch.full((B, max_tokens), m.blank, dtype=torch.int32, device=dev)
        frame_idx = torch.zeros(B, dtype=torch.int32, device=dev)
        tok_idx = torch.full((B,), -1, dtype=torch.int32, device=dev)
        per_frame = torch.zeros(B, dtype=torch.int32, device=dev)
        active = torch.ones(1, dtype=torch.int32, device=dev)
        h_new, c_new = torch.empty(B, P, dtype=f32, device=dev), torch.empty(B, P, dtype=f32, device=dev)
        zbuf, logits = torch.empty(B, J, dtype=f32, device=dev), torch.empty(B, V, dtype=f32, device=dev)
        Wk, Wrk, Wjp, Wv = ps.p2d("pred/lstm/k"), ps.p2d("pred/lstm/rk"), ps.p2d("joint/pred/w"), ps.p2d("joint/vocab/w")
        lng, lnb = (ps.p("pred/ln/g"), ps.p("pred/ln/b")) if c.prediction_layer_norm else (None, None)
        fused = B <= 64 and m.decode_fused
        if fused and self._packed is None:
            self._packed = K.decode_pack(ps.p("pred/emb"), Wk, Wrk, Wjp, Wv)  # (inference session: the weights are constants)
        it, max_iters = 0, max(nv_host) * mtpf + 1  # every iteration of an active row advances its frame or appends a token
        need = max(nv_host)
        while it < max_iters:
            n = min(max(need, 4), max_iters - it)
            if fused and self.detail:
                fused = K.decode_steps_detail(ps.p("pred/emb"), Wk, Wrk, ps.p("pred/lstm/b"), lng, lnb, Wjp, ps.p("joint/pred/b"), Wv,
                                              ps.p("joint/vocab/b"), encj, nvalid, frame_idx, tok_idx, self.prev_tok, self.h, self.c, active, h_new,
                                              c_new, zbuf, logits, tokens, per_frame, *detail, max_tokens, m.blank, 2, mtpf, n, packed=self._packed)
            elif fused:
                fused = K.decode_steps(ps.p("pred/emb"), Wk, Wrk, ps.p("pred/lstm/b"), lng, lnb, Wjp, ps.p("joint/pred/b"), Wv, ps.p("joint/vocab/b"),
                                       encj, nvalid, frame_idx, tok_idx, self.prev_tok, self.h, self.c, active, h_new, c_new, zbuf, logits, tokens,
                                       per_frame, max_tokens, m.blank, 2, mtpf, n, packed=self._packed)
            if not fused:
                ecur = torch.empty(B, J, dtype=f32, device=dev)
                xg, hr, pj = torch.empty(B, 4 * P, dtype=f32, device=dev), torch.empty(B, 4 * P, dtype=f32, device=dev), torch.empty(B, J, dtype=f32, device=dev)
                for _ in range(n):
                    K.decode_prepare(encj, nvalid, frame_idx, tok_idx, active, ecur, max_tokens, 2)
                    emb = K.embedding_fwd(self.prev_tok, ps.p("pred/emb"), f32)
                    K.matmul(emb, Wk, bias=ps.p("pred/lstm/b"), out=xg)
                    K.gemm(self.h, Wrk, hr, B, 4 * P, P, P, 4 * P, 4 * P)
                    K.lstm_step_fwd(xg, hr, self.h, self.c, None, 0, None, c_new, h_new, None, B, P)
                    y = K.layernorm_fwd(h_new, lng, lnb, save_stats=False)[0] if c.prediction_layer_norm else h_new
                    K.matmul(y, Wjp, bias=ps.p("joint/pred/b"), out=pj)
                    z = K.joint_fwd(ecur.view(B, 1, J), pj.view(B, 1, J))
                    K.matmul(z.view(B, J), Wv, bias=ps.p("joint/vocab/b"), out=logits)
                    if self.detail:
                        K.decode_update_detail(logits, active, nvalid, frame_idx, self.prev_tok, tok_idx, tokens, per_frame, h_new, c_new, self.h,
                                               self.c, *detail, max_tokens, m.blank, 2, mtpf)
                    else:
                        K.decode_update(logits, active, nvalid, frame_idx, self.prev_tok, tok_idx, tokens, per_frame, h_new, c_new, self.h, self.c,
                                        max_tokens, m.blank, 2, mtpf)
            it += n
            left = (nvalid - frame_idx).clamp_(min=0).max()
            need = int(left.item())  # (one sync per batch of iterations)
            if need == 0:
                break
        if self.detail:
            (toks, frames), (logp, ent), tl = ibuf.cpu().tolist(), fbuf.cpu().tolist(), tok_idx.cpu().tolist()  # (plain lists: the rows are short)
            for b in range(B):
                n = tl[b] + 1
                # the kernel's frame is chunk-local: self.frames[b] is the stream's frame count in front of this chunk
                self.record[b].extend(toks[b][:n], [f + self.frames[b] for f in frames[b][:n]], None, logp[b][:n], ent[b][:n])
            return [toks[b][:tl[b] + 1] for b in range(B)]
        th, tl = tokens.cpu(), tok_idx.cpu()  # the fetch of the new tokens: the one host round trip of a chunk besides the loop check
        return [th[b, :int(tl[b]) + 1].tolist() for b in range(B)]

    def _search_ctc(self, enc, nvalid):
        m = self.model
        ps = m.ps
        B, C, _ = enc.shape
        logits = K.matmul(self._enc32(enc), ps.p2d("dec/logits/w"), bias=ps.p("dec/logits/b")).view(B, C, m.cfg.vocab_size)
        if self.detail:
            return self._ctc_detail(logits, nvalid)
        tokens, tlen = K.ctc_greedy_decode_carry(logits, nvalid, self.last_class, blank=m.blank)
        th, tl = tokens.cpu(), tlen.cpu()
        return [th[b, :int(tl[b])].tolist() for b in range(B)]

    def _ctc_detail(self, logits, nvalid, final=None):
        """One launch of tfasr_ctc_greedy_decode_carry_detail on the session's carried state, its result merged into the record: column 0
        updates the token that was open, columns 1 .. n are appended -> the new tokens per stream."""
        B, C, _ = logits.shape
        out = K.ctc_greedy_decode_carry_detail(logits, nvalid, self.ctc_state, final, blank=self.model.blank, packed=True)
        (toks, starts, ends), (logp, ent), tl = (t.cpu().tolist() for t in out)  # (plain lists: the rows are short)
        new = []
        for b in range(B):
            rec, cols = self.record[b], slice(1, tl[b] + 1)
            if starts[b][0] >= 0:
                rec.update_last(ends[b][0], logp[b][0], ent[b][0])
            rec.extend(toks[b][cols], starts[b][cols], ends[b][cols], logp[b][cols], ent[b][cols])
            new.append(toks[b][cols])
        return new

    # ------------------------------------------------------------------------------------------- public
    def accept(self, pcm, lengths=None):
        """pcm [B, n] f32 (or [n] with batch_size 1), lengths [B] real samples per row (default n): buffers them, runs every chunk that
        is complete for at least one stream, continues the search -> StreamOutput."""
        x = pcm.detach().cpu().numpy() if isinstance(pcm, torch.Tensor) else np.asarray(pcm)
        x = np.asarray(x, np.float32)
        if x.ndim == 1:
            x = x[None]
        if x.shape[0] != self.B:
            raise ValueError(f"accept takes [{self.B}, n] samples")
        lens = [x.shape[1]] * self.B if lengths is None else [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        for b in range(self.B):
            if lens[b] > 0 and self.finished[b]:
                raise RuntimeError(f"stream {b} is finished: reset it before it takes another utterance")
        self._check_capacity(more=[max(n, 0) for n in lens])
        for b in range(self.B):
            if lens[b] > 0:
                self.buf[b] = np.concatenate([self.buf[b], x[b, :lens[b]]])
                self.total[b] += lens[b]
        return self._run()

    def finish(self, rows=None):
        """Pad the tail of the given streams (default: all) as pad_end=True does, run their last (partial) chunk -> StreamOutput; those
        streams then refuse accept until reset."""
        rows = [b for b in (range(self.B) if rows is None else rows) if not self.finished[b]]
        self._check_capacity(flush_rows=set(rows))
        out = self._run(flush_rows=set(rows))
        for b in rows:
            self.finished[b] = True
            self.buf[b] = np.zeros(0, np.float32)
        return out

    # ------------------------------------------------------------------------------------------- detail sessions
    def _check_detail(self, detail):
        if detail and getattr(self, "commit_horizon", None):
            raise ValueError("stream: a detail session is greedy and takes no commit_horizon")
        if detail and getattr(self, "lm_tables", None) is not None:
            raise ValueError("stream: lm belongs to a beam session; detail sessions are greedy")
        if detail and self.beam_width:
            raise ValueError("stream: detail=True belongs to the greedy session (beam_width=0): beam sessions keep their outputs, their "
                             "searches record no token times or confidences")
        return bool(detail)

    def detailed(self):
        """This session, which has taken no audio yet, as a detail session (what model.stream_detailed returns) -> self."""
        if any(self.total) or self.chunks_run:
            raise RuntimeError("stream: detailed() opens a detail session and comes before the first accept()")
        self.detail = self._check_detail(True)
        self._init_rows(range(self.B), first=True)  # the search state of a detail session (the record; the CTC head's carried state)
        return self

    def _need_detail(self, what):
        if not self.detail:
            raise ValueError(f"{what} needs a detail session: open it with model.stream_detailed(...)")

    def open_tokens(self):
        """[B] bool: the stream's last token is a CTC run that reached the last frame seen, so its end and its values can still change
        (never for a transducer, never after finish())."""
        self._need_detail("open_tokens()")
        return torch.tensor([r.open for r in self.record], dtype=torch.bool)

    def recognized(self, rows=None):
        """Everything the given streams (default: all) have emitted since their reset -> schemas.RecognizeOutput on the host, row i =
        stream rows[i], what model.recognize_detailed gives the utterance so far (schemas.token_times / token_confidences / word_details
        read it).  Every closed token holds its final values; a CTC stream's open token (open_tokens()) holds ends = the frames seen so far
        and the sum / the mean over its frames so far.  scores: transducer = the sum of the tokens' log_probs, CTC = the carried path score."""
        self._need_detail("recognized()")
        from .schemas import PredictOutput, RecognizeOutput

        rows = list(range(self.B)) if rows is None else [int(b) for b in rows]
        recs = [self.record[b] for b in rows]
        R, W = len(rows), max([len(r.tokens) for r in recs] + [1])
        tokens = torch.full((R, W), self.model.blank, dtype=torch.int32)
        frames, ends = torch.full((R, W), -1, dtype=torch.int32), torch.full((R, W), -1, dtype=torch.int32)
        logp, ent = torch.zeros(R, W, dtype=torch.float32), torch.zeros(R, W, dtype=torch.float32)
        for i, (b, r) in enumerate(zip(rows, recs)):
            n = len(r.tokens)
            if n:
                tokens[i, :n] = torch.tensor(r.tokens, dtype=torch.int32)
                frames[i, :n] = torch.tensor(r.frames, dtype=torch.int32)
                ends[i, :n] = torch.tensor(r.ends[:-1] + [self.frames[b] if r.open else r.ends[-1]], dtype=torch.int32)
                logp[i, :n] = torch.tensor(r.logp, dtype=torch.float32)
                ent[i, :n] = torch.tensor(r.ent, dtype=torch.float32)
        scores = self.ctc_state.score.cpu()[rows] if self.ctc else logp.sum(1)
        predict = PredictOutput(tokens=tokens, next_tokens=None, next_encoder_states=None, next_decoder_states=None)
        return RecognizeOutput(predict, frames, ends if self.ctc else None, logp, ent, scores, self.model.seconds_per_frame,
                               self.model.cfg.vocab_size)

    def trailing_blank_frames(self):
        """[B] int32: the encoder frames since the end of each stream's last token (CTC: one past its run, 0 while the run is open;
        transducer: after the frame that emitted it); the whole stream when nothing was emitted.  What an endpointing rule reads."""
        self._need_detail("trailing_blank_frames()")
        return torch.tensor([0 if r.open else self.frames[b] - (r.ends[-1] if r.ends else 0) for b, r in enumerate(self.record)],
                            dtype=torch.int32)
