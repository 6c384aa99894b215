"""Model configuration with the reference's keyword surface.

`ConformerConfig.from_reference(config)` accepts the `model_config.config` mapping of
examples/models/transducer/conformer/small.yml.j2:3-69 (= the kwargs of
tensorflow_asr/models/transducer/conformer.py:23-79) unchanged.  `conformer_s()` is that file's values;
`conformer_m()` is the Conformer-M of arXiv:2005.08100 Table 1 expressed through the same keys (the reference ships
no M config: SURVEY.md §0.1).
"""
import math
from dataclasses import dataclass, field


def speech_kwargs(sc, log_bases=("e",), feature_types=("log_mel_spectrogram",)):
    """`speech_config` of the reference's YAML (FeatureExtraction.__init__, models/layers/feature_extraction.py:32-130) -> the front-end
    fields of ConformerConfig.  Options the MI355X front end does not implement fail loudly instead of being ignored; the epsilon range
    check is the reference's (feature_extraction.py:113).  log_bases: the values of `log_base` the caller's model handles (the result
    does not carry the base: a model that accepts "10" reads it from the mapping itself).  feature_types: the values of `feature_type` the
    caller's model handles (likewise not carried)."""
    sc = dict(sc or {})
    only = {"feature_type": tuple(feature_types), "pad_end": (True,), "use_librosa_like_stft": (False,), "log_base": tuple(log_bases),
            "normalize_signal": (False,), "normalize_zscore": (False,), "normalize_min_max": (False,), "padding": (0,)}
    for k, ok in only.items():
        if k in sc and sc[k] not in ok:
            raise NotImplementedError(f"speech_config.{k}={sc[k]!r}: only {ok} is on the MI355X hot path")
    nfft = sc.get("nfft", 512)
    if nfft is None:  # the reference falls back to the frame length (feature_extraction.py:121)
        nfft = int(round(sc.get("sample_rate", 16000) * sc.get("frame_ms", 25) / 1000.0))
    if nfft != 512 or int(round(sc.get("sample_rate", 16000) * sc.get("frame_ms", 25) / 1000.0)) > 512:
        raise NotImplementedError(f"speech_config: nfft={nfft} / frame_ms={sc.get('frame_ms', 25)}: the front-end kernel is a 512-point transform (frames of up to 512 samples)")
    eps = float(sc.get("epsilon", 1e-6))
    assert eps > 1e-9 and eps <= 0.001, "epsilon must be in (1e-9, 0.001]"
    return dict(sample_rate=sc.get("sample_rate", 16000), frame_ms=sc.get("frame_ms", 25), stride_ms=sc.get("stride_ms", 10), nfft=nfft,
                num_feature_bins=sc.get("num_feature_bins", 80), preemphasis=sc.get("preemphasis", 0.97), epsilon=eps,
                lower_edge_hertz=float(sc.get("lower_edge_hertz", 0.0)), upper_edge_hertz=float(sc.get("upper_edge_hertz", 8000.0)))


@dataclass
class ConformerConfig:
    # speech_config (models/layers/feature_extraction.py:34-55)
    sample_rate: int = 16000
    frame_ms: int = 25
    stride_ms: int = 10
    nfft: int = 512
    num_feature_bins: int = 80
    preemphasis: float = 0.97
    epsilon: float = 1e-6
    lower_edge_hertz: float = 0.0
    upper_edge_hertz: float = 8000.0
    # augmentation (small.yml.j2:11-24)
    time_masking: dict = field(default_factory=lambda: dict(prob=1.0, num_masks=10, mask_factor=-1, p_upperbound=0.05, mask_value=0))
    freq_masking: dict = field(default_factory=lambda: dict(prob=1.0, num_masks=1, mask_factor=27, mask_value=0))
    # encoder
    filters: int = 144
    dmodel: int = 144
    num_blocks: int = 16
    head_size: int = 36
    num_heads: int = 4
    kernel_size: int = 31
    ffm_scale: int = 4
    ffm_residual: float = 0.5
    mhsam_residual: float = 1.0
    convm_residual: float = 1.0
    dropout: float = 0.1
    use_attention_auto_mask: bool = True
    # streaming Conformer (examples/models/transducer/conformer/small-streaming.yml.j2:33,38-39): chunked attention mask
    # (multihead_attention.py:104-143,331-345) and LayerNormalization after the depthwise conv (encoders/conformer.py:334-340)
    chunk_size: int = None
    history_size: int = None
    convm_dw_norm: str = "batch"
    sub_norm: str = "batch"  # Conv2dSubsampling `norms` (subsampling.py:197-213): "batch" (small.yml.j2) or "layer" (small-streaming.yml.j2)
    # encoder_mhsam_use_attention_bias: True (examples/models/ctc/conformer/small.yml.j2:45): per-layer content / positional
    # attention biases (multihead_attention.py:522-538) instead of the encoder-level shared pair (encoders/conformer.py:647-663)
    mhsam_use_attention_bias: bool = False
    # model head: "transducer" (prediction + joint networks) or "ctc" (models/ctc/conformer.py:21-47: one Dense(vocab) decoder)
    head: str = "transducer"
    # prediction / joint
    embed_dim: int = 320
    rnn_units: int = 320
    joint_dim: int = 320
    vocab_size: int = 1000
    blank: int = 0
    l2: float = 1e-6
    prediction_layer_norm: bool = True
    # encoder family: "conformer" (default) or "contextnet" (models/encoders/contextnet.py)
    encoder: str = "conformer"
    contextnet_blocks: list = None   # [dict(nlayers, kernel_size, filters, strides, residual)], the yml's encoder_blocks
    contextnet_alpha: float = 1.0

    @property
    def frame_length(self):
        return int(round(self.sample_rate * self.frame_ms / 1000.0))

    @property
    def frame_step(self):
        return int(round(self.sample_rate * self.stride_ms / 1000.0))

    @property
    def time_reduction_factor(self):
        if self.encoder == "contextnet":
            f = 1
            for b in self.contextnet_blocks:
                f *= int(b.get("strides", 1))
            return f
        return 4

    @classmethod
    def from_reference(cls, config: dict, class_name: str = None):
        """Map the reference's Conformer kwargs (models/transducer/conformer.py:23-79; models/ctc/conformer.py:57-100 when
        `class_name` is the YAML's "tensorflow_asr.models.ctc.conformer>Conformer") onto this dataclass."""
        c = dict(config)
        sc = dict(c.get("speech_config", {}))
        aug = (sc.get("augmentation_config") or {}).get("feature_augment", {}) or {}
        sub = (c.get("encoder_subsampling") or {}).get("config", {})
        unsupported = {
            "encoder_mha_type": ("relmha",), "encoder_padding": ("causal",), "prediction_rnn_type": ("lstm",),
            "prediction_num_rnns": (1,), "joint_activation": ("tanh",), "joint_mode": ("add",),
            "encoder_convm_dw_norm_type": ("batch", "layer"), "prediction_label_encode_mode": ("embedding",),
            "encoder_memory_length": (None,), "encoder_use_attention_causal_mask": (False,),
            # constructor options of models/transducer/conformer.py:23-77 (models/ctc/conformer.py for the CTC head) that change the
            # network and are not built: a non-default value must not be ignored silently
            "encoder_interleave_relpe": (True,), "encoder_mhsam_causal": (False,), "encoder_convm_scale_factor": (2,),
            "encoder_convm_use_group_conv": (False,), "encoder_module_norm_position": ("pre",), "encoder_block_norm_position": ("post",),
            "encoder_trainable": (True,), "prediction_trainable": (True,), "joint_trainable": (True,),
            "prediction_projection_units": (0,), "prejoint_encoder_linear": (True,), "prejoint_prediction_linear": (True,),
            "postjoint_linear": (False,), "bias_regularizer": (None,), "activity_regularizer": (None,), "recurrent_regularizer": (None,),
        }
        if "prediction_layer_norm" in c and not c["prediction_layer_norm"] and not (class_name and ".ctc." in class_name):
            raise NotImplementedError("prediction_layer_norm=False: the Conformer transducer's prediction network ends in a LayerNorm here "
                                      "(base_transducer.py:123-132 with the YAML default)")
        for k, ok in unsupported.items():
            if k in c and c[k] not in ok:
                raise NotImplementedError(f"{k}={c[k]!r}: only {ok} is on the MI355X hot path")
        # A key the mapping omits takes Conv2dSubsampling's OWN default (subsampling.py:163-176: strides [[2, 1], [2, 1]], kernels
        # [[3, 3], [3, 3]], paddings causal, norms none, activations relu) - which is not the network of small.yml.j2 and is not built, so
        # an incomplete mapping raises instead of silently becoming BatchNorm + swish.  No `encoder_subsampling` at all (the
        # reference's constructor requires one, models/transducer/conformer.py:28): the shipped small.yml.j2 block.
        ref_def = dict(kernels=[[3, 3], [3, 3]], strides=[[2, 1], [2, 1]], paddings=["causal", "causal"], norms=["none", "none"],
                       activations=["relu", "relu"])
        yml_def = dict(kernels=[3, 3], strides=[2, 2], paddings=["causal", "causal"], norms=["batch", "batch"], activations=["swish", "swish"])
        getd = (lambda k: sub.get(k, ref_def[k])) if sub else (lambda k: yml_def[k])

        def _pairs(v):  # [3, 3] (both layers 3 -> keras broadcasts an int to both axes) and [[3, 3], [3, 3]] describe the same convolutions
            return [list(x) if isinstance(x, (list, tuple)) else [x, x] for x in v]

        if _pairs(getd("kernels")) != [[3, 3], [3, 3]] or _pairs(getd("strides")) != [[2, 2], [2, 2]]:
            raise NotImplementedError(f"encoder_subsampling kernels={getd('kernels')} strides={getd('strides')}: only the 3x3 stride-2 causal "
                                      f"Conv2dSubsampling of small.yml.j2:26-33 is supported")
        norms = [str(n) for n in getd("norms")]
        if norms not in (["batch", "batch"], ["layer", "layer"]):
            raise NotImplementedError(f"encoder_subsampling.norms={norms}: both blocks 'batch' (small.yml.j2:31) or both 'layer' "
                                      f"(small-streaming.yml.j2) are built (subsampling.py:197-213)")
        if [str(a) for a in getd("activations")] not in (["swish", "swish"], ["silu", "silu"]):
            raise NotImplementedError(f"encoder_subsampling.activations={getd('activations')}: only swish (small.yml.j2:32)")
        if [str(a) for a in getd("paddings")] != ["causal", "causal"]:
            raise NotImplementedError(f"encoder_subsampling.paddings={getd('paddings')}: only causal (small.yml.j2:30)")
        reg = c.get("kernel_regularizer") or {}
        l2 = float((reg.get("config") or {}).get("l2", 1e-6)) if isinstance(reg, dict) else 1e-6
        kw = dict(
            **speech_kwargs(sc),
            filters=(sub.get("filters") or [c.get("encoder_dmodel", 144)])[0], dmodel=c.get("encoder_dmodel", 144),
            num_blocks=c.get("encoder_num_blocks", 16), head_size=c.get("encoder_head_size", 36),
            num_heads=c.get("encoder_num_heads", 4), kernel_size=c.get("encoder_kernel_size", 31),
            ffm_scale=c.get("encoder_ffm_scale_factor", 4), ffm_residual=c.get("encoder_ffm_residual_factor", 0.5),
            mhsam_residual=c.get("encoder_mhsam_residual_factor", 1.0), convm_residual=c.get("encoder_convm_residual_factor", 1.0),
            dropout=c.get("encoder_dropout", 0.1), use_attention_auto_mask=c.get("encoder_use_attention_auto_mask", True),
            embed_dim=c.get("prediction_embed_dim", 512), rnn_units=c.get("prediction_rnn_units", 320),
            joint_dim=c.get("joint_dim", 1024), vocab_size=int(c.get("vocab_size", 1000)), blank=c.get("blank", 0), l2=l2,
            chunk_size=c.get("encoder_chunk_size"), history_size=c.get("encoder_history_size"),
            convm_dw_norm=c.get("encoder_convm_dw_norm_type", "batch"), sub_norm=norms[0],
            mhsam_use_attention_bias=bool(c.get("encoder_mhsam_use_attention_bias", False)))
        if class_name and ".ctc." in class_name:
            kw["head"] = "ctc"
        if (kw["chunk_size"] is None) != (kw["history_size"] is None):  # multihead_attention.py:339 needs both
            kw["chunk_size"] = kw["history_size"] = None
        if "time_masking" in aug:
            kw["time_masking"] = dict(aug["time_masking"])
        if "freq_masking" in aug:
            kw["freq_masking"] = dict(aug["freq_masking"])
        return cls(**kw)


def conformer_ctc_s(vocab_size=1000, **over):
    """examples/models/ctc/conformer/small.yml.j2:26-46: d=176, 4 heads of 44, per-layer attention biases, Dense(vocab) decoder."""
    kw = dict(filters=176, dmodel=176, head_size=44, num_heads=4, mhsam_use_attention_bias=True, head="ctc", vocab_size=vocab_size)
    kw.update(over)
    return ConformerConfig(**kw)


def conformer_s(vocab_size=1000, **over):
    return ConformerConfig(vocab_size=vocab_size, **over)


def conformer_m(vocab_size=1000, **over):
    kw = dict(filters=256, dmodel=256, head_size=64, num_heads=4, embed_dim=640, rnn_units=640, joint_dim=640, vocab_size=vocab_size)
    kw.update(over)
    return ConformerConfig(**kw)


CONTEXTNET_BLOCKS = (  # examples/models/transducer/contextnet/small.yml.j2:25-190 (nlayers, kernel, filters, stride, residual)
    [(1, 5, 256, 1, False)] + [(5, 5, 256, 1, True)] * 2 + [(5, 5, 256, 2, True)] + [(5, 5, 256, 1, True)] * 3 + [(5, 5, 256, 2, True)]
    + [(5, 5, 256, 1, True)] * 3 + [(5, 5, 512, 1, True)] * 3 + [(5, 5, 512, 2, True)] + [(5, 5, 512, 1, True)] * 7 + [(1, 5, 640, 1, False)])


def _cn_blocks(spec):
    return [dict(nlayers=n, kernel_size=k, filters=f, strides=s, residual=r) for n, k, f, s, r in spec]


def contextnet(vocab_size=1000, alpha=0.5, **over):
    """The reference's ContextNet transducer (contextnet/small.yml.j2: alpha 0.5, 23 blocks, time reduction 8, prediction
    LSTM 512 without LayerNorm, joint 512); alpha 1 / 2 give the paper's M / L widths."""
    blocks = _cn_blocks(CONTEXTNET_BLOCKS)
    kw = dict(encoder="contextnet", contextnet_blocks=blocks, contextnet_alpha=alpha, dmodel=int(blocks[-1]["filters"] * alpha), embed_dim=640,
              rnn_units=512, joint_dim=512, prediction_layer_norm=False, vocab_size=vocab_size, dropout=0.0)
    kw.update(over)
    return ConformerConfig(**kw)


def contextnet_from_reference(config: dict):
    """The reference's ContextNet kwargs (models/transducer/contextnet.py:23-52; contextnet/small.yml.j2:1-220) -> config."""
    c = dict(config)
    for k, ok in {"prediction_rnn_type": ("lstm",), "prediction_num_rnns": (1,), "joint_activation": ("tanh",), "joint_mode": ("add",),
                  "prediction_label_encode_mode": ("embedding",), "prediction_projection_units": (0,)}.items():
        if k in c and c[k] not in ok:
            raise NotImplementedError(f"{k}={c[k]!r}: only {ok} is on the MI355X hot path")
    blocks = []
    for b in c["encoder_blocks"]:
        if str(b.get("activation", "silu")) not in ("silu", "swish") or str(b.get("padding", "causal")) != "causal":
            raise NotImplementedError(f"ContextNet block {b}: only silu activations / causal padding are built")
        blocks.append(dict(nlayers=int(b["nlayers"]), kernel_size=int(b["kernel_size"]), filters=int(b["filters"]), strides=int(b.get("strides", 1)),
                           residual=bool(b.get("residual", True))))
    alpha = float(c.get("encoder_alpha", 0.5))
    sc = dict(c.get("speech_config", {}))
    aug = (sc.get("augmentation_config") or {}).get("feature_augment", {}) or {}
    reg = c.get("kernel_regularizer") or {}
    kw = dict(encoder="contextnet", contextnet_blocks=blocks, contextnet_alpha=alpha, dmodel=int(blocks[-1]["filters"] * alpha),
              embed_dim=c.get("prediction_embed_dim", 512), rnn_units=c.get("prediction_rnn_units", 320), joint_dim=c.get("joint_dim", 1024),
              prediction_layer_norm=bool(c.get("prediction_layer_norm", True)), vocab_size=int(c.get("vocab_size", 1000)), blank=c.get("blank", 0),
              dropout=0.0, l2=float((reg.get("config") or {}).get("l2", 1e-6)) if isinstance(reg, dict) else 1e-6,
              **speech_kwargs(sc))
    if "time_masking" in aug:
        kw["time_masking"] = dict(aug["time_masking"])
    if "freq_masking" in aug:
        kw["freq_masking"] = dict(aug["freq_masking"])
    return ConformerConfig(**kw)


def contextnet_tiny(vocab_size=29, **over):
    blocks = _cn_blocks([(1, 5, 32, 1, False), (3, 5, 32, 1, True), (3, 5, 32, 2, True), (2, 3, 48, 2, True), (1, 5, 64, 1, False)])
    kw = dict(encoder="contextnet", contextnet_blocks=blocks, contextnet_alpha=0.5, dmodel=32, embed_dim=24, rnn_units=24, joint_dim=40,
              prediction_layer_norm=False, vocab_size=vocab_size, dropout=0.0)
    kw.update(over)
    return ConformerConfig(**kw)


def conformer_tiny(vocab_size=29, **over):
    kw = dict(dropout=0.0, filters=32, dmodel=32, head_size=8, num_heads=4, embed_dim=24, rnn_units=24, joint_dim=40, num_blocks=2,
              kernel_size=7, vocab_size=vocab_size)
    kw.update(over)
    return ConformerConfig(**kw)


# ------------------------------------------------------------------------------------------------------------------ Jasper (CTC)
@dataclass
class JasperConfig:
    """The keyword surface of tensorflow_asr.models.ctc.jasper.Jasper (models/ctc/jasper.py:61-92) with `speech_config` flattened as in
    ConformerConfig.  Inference only: the dropout rates are kept for the record and never applied."""
    # speech_config
    sample_rate: int = 16000
    frame_ms: int = 25
    stride_ms: int = 10
    nfft: int = 512
    num_feature_bins: int = 80
    preemphasis: float = 0.97
    epsilon: float = 1e-6
    lower_edge_hertz: float = 0.0
    upper_edge_hertz: float = 8000.0
    log_base: str = "10"
    # encoder (models/encoders/jasper.py:231-256; values: examples/models/ctc/jasper/base.yml.j2:13-32)
    dense: bool = True
    padding: str = "causal"
    first_additional_block_channels: int = 256
    first_additional_block_kernels: int = 11
    first_additional_block_strides: int = 2
    first_additional_block_dilation: int = 1
    first_additional_block_dropout: float = 0.2
    nsubblocks: int = 3
    block_channels: list = field(default_factory=lambda: [256, 384, 512, 640, 768])
    block_kernels: list = field(default_factory=lambda: [11, 13, 17, 21, 25])
    block_dropout: list = field(default_factory=lambda: [0.2, 0.2, 0.2, 0.3, 0.3])
    second_additional_block_channels: int = 896
    second_additional_block_kernels: int = 1
    second_additional_block_strides: int = 1
    second_additional_block_dilation: int = 2
    second_additional_block_dropout: float = 0.4
    third_additional_block_channels: int = 1024
    third_additional_block_kernels: int = 1
    third_additional_block_strides: int = 1
    third_additional_block_dilation: int = 1
    third_additional_block_dropout: float = 0.4
    vocab_size: int = 1000
    blank: int = 0
    l2: float = 1e-6
    # what the shared model code reads from every config
    encoder: str = "jasper"
    head: str = "ctc"
    dropout: float = 0.0
    chunk_size: int = None
    history_size: int = None
    time_masking: dict = None
    freq_masking: dict = None
    head_size: int = 64   # (no attention: the values only keep ParamStore's head / filter padding off)
    num_heads: int = 1
    filters: int = 64

    def __post_init__(self):
        self.block_channels, self.block_kernels = [int(v) for v in self.block_channels], [int(v) for v in self.block_kernels]
        self.block_dropout = [float(v) for v in self.block_dropout]
        if not len(self.block_channels) == len(self.block_kernels) == len(self.block_dropout):  # encoders/jasper.py:260
            raise ValueError("block_channels, block_kernels and block_dropout must have one entry per block")
        if str(self.padding) != "causal":
            raise NotImplementedError(f"padding={self.padding!r}: only causal convolutions are on the MI355X hot path")
        if self.log_base not in ("e", "10"):
            raise NotImplementedError(f"log_base={self.log_base!r}: 'e' or '10'")
        if int(self.nsubblocks) < 1:
            raise ValueError("nsubblocks must be >= 1")
        s1 = int(self.first_additional_block_strides)
        if s1 not in (1, 2):
            raise NotImplementedError(f"first_additional_block_strides={s1}: the Conv1D kernel strides by 1 or 2")
        for which in ("second", "third"):
            if int(getattr(self, which + "_additional_block_strides")) != 1:
                raise NotImplementedError(f"{which}_additional_block_strides != 1: only the first block may stride (base.yml.j2:16,25,30)")
        chans = [self.num_feature_bins, self.first_additional_block_channels, *self.block_channels, self.second_additional_block_channels,
                 self.third_additional_block_channels]
        if any(int(c) <= 0 or int(c) % 16 for c in chans):
            raise NotImplementedError(f"channel counts {chans} (feature bins included): the Conv1D kernel takes multiples of 16")
        for k, d in [(self.first_additional_block_kernels, self.first_additional_block_dilation), *((k, 1) for k in self.block_kernels),
                     (self.second_additional_block_kernels, self.second_additional_block_dilation),
                     (self.third_additional_block_kernels, self.third_additional_block_dilation)]:
            if not 1 <= int(k) <= 32 or int(d) < 1 or (int(k) - 1) * int(d) > 256:
                raise NotImplementedError(f"kernel {k} / dilation {d}: the Conv1D kernel takes 1..32 taps spanning at most 256 rows")

    @property
    def dmodel(self):
        return int(self.third_additional_block_channels)

    @property
    def frame_length(self):
        return int(round(self.sample_rate * self.frame_ms / 1000.0))

    @property
    def frame_step(self):
        return int(round(self.sample_rate * self.stride_ms / 1000.0))

    @property
    def time_reduction_factor(self):
        """encoders/jasper.py:318-320: the product of the three additional blocks' strides"""
        return (int(self.first_additional_block_strides) * int(self.second_additional_block_strides)
                * int(self.third_additional_block_strides))

    def encoder_length(self, n):
        """math_util.get_reduced_length: ceil(n / time_reduction_factor)"""
        return -(-int(n) // self.time_reduction_factor)


def jasper(vocab_size=1000, layout="base", **over):
    """examples/models/ctc/jasper/base.yml.j2 (5 blocks of 3 sub-blocks, dense residuals); layout="10x5": the 10-block, 5-sub-block
    network of arXiv:1904.03288 Table 1 that BASELINE.json names, through the same keys."""
    kw = dict(vocab_size=vocab_size)
    if layout == "10x5":
        kw.update(nsubblocks=5, block_channels=[256, 256, 384, 384, 512, 512, 640, 640, 768, 768],
                  block_kernels=[11, 11, 13, 13, 17, 17, 21, 21, 25, 25], block_dropout=[0.2, 0.2, 0.2, 0.2, 0.2, 0.2, 0.3, 0.3, 0.3, 0.3])
    elif layout != "base":
        raise ValueError(f"layout {layout!r}: 'base' or '10x5'")
    kw.update(over)
    return JasperConfig(**kw)


def jasper_tiny(vocab_size=29, **over):
    kw = dict(vocab_size=vocab_size, nsubblocks=3, block_channels=[64, 96], block_kernels=[11, 13], block_dropout=[0.0, 0.0],
              first_additional_block_channels=48, first_additional_block_kernels=11, second_additional_block_channels=128,
              third_additional_block_channels=160)
    kw.update(over)
    return JasperConfig(**kw)


def jasper_from_reference(config: dict):
    """The YAML's `model_config.config` of tensorflow_asr.models.ctc.jasper>Jasper (base.yml.j2:3-38) -> JasperConfig.  Options that are
    not built raise (JasperConfig.__post_init__ and speech_kwargs); a regulariser other than l2 on the kernels, too."""
    c = dict(config)
    sc = dict(c.get("speech_config", {}))
    for k in ("bias_regularizer", "activity_regularizer"):
        if c.get(k) is not None:
            raise NotImplementedError(f"{k}={c[k]!r}: not built")
    reg = c.get("kernel_regularizer") or {}
    kw = dict(**speech_kwargs(sc, log_bases=("e", "10")), log_base=str(sc.get("log_base", "e")),
              l2=float((reg.get("config") or {}).get("l2", 1e-6)) if isinstance(reg, dict) else 1e-6)
    fields = {f for f in JasperConfig.__dataclass_fields__}
    for k, v in c.items():
        if k in ("speech_config", "kernel_regularizer", "bias_regularizer", "activity_regularizer", "name"):
            continue
        if k not in fields or k in ("encoder", "head", "head_size", "num_heads", "filters", "chunk_size", "history_size"):
            raise NotImplementedError(f"{k}={v!r}: not a keyword of models/ctc/jasper.py:61-92 that is built here")
        kw[k] = v
    return JasperConfig(**kw)


# ------------------------------------------------------------------------------------------------------------------ DeepSpeech2 (CTC)
@dataclass
class DeepSpeech2Config:
    """The keyword surface of tensorflow_asr.models.ctc.deepspeech2.DeepSpeech2 (models/ctc/deepspeech2.py:58-89) with `speech_config`
    flattened as in ConformerConfig.  The defaults are the CLASS's defaults (:63-83); deepspeech2() holds the shipped YAML's values.
    Inference only: the dropout rates and regularisers are kept for the record and never applied."""
    # speech_config
    sample_rate: int = 16000
    frame_ms: int = 25
    stride_ms: int = 10
    nfft: int = 512
    num_feature_bins: int = 80
    preemphasis: float = 0.97
    epsilon: float = 1e-6
    lower_edge_hertz: float = 0.0
    upper_edge_hertz: float = 8000.0
    feature_type: str = "log_mel_spectrogram"
    # encoder (models/encoders/deepspeech2.py:417-443)
    conv_type: str = "conv2d"
    conv_kernels: list = field(default_factory=lambda: [[11, 41], [11, 21], [11, 21]])
    conv_strides: list = field(default_factory=lambda: [[3, 2], [1, 2], [1, 2]])
    conv_filters: list = field(default_factory=lambda: [32, 32, 96])
    conv_padding: str = "same"
    conv_activation: str = "relu"
    conv_initializer: str = None
    rnn_nlayers: int = 5
    rnn_type: str = "lstm"
    rnn_units: int = 1024
    rnn_bidirectional: bool = True
    rnn_unroll: bool = False
    rnn_rowconv: int = 0
    rnn_rowconv_activation: str = "relu"
    rnn_dropout: float = 0.1
    rnn_initializer: str = None
    fc_nlayers: int = 0
    fc_units: int = 1024
    fc_activation: str = "relu"
    fc_dropout: float = 0.1
    fc_initializer: str = None
    initializer: str = "glorot_uniform"
    vocab_size: int = 1000
    blank: int = 0
    l2: float = 0.0
    bias_l2: float = 0.0
    # what the shared model code reads from every config
    encoder: str = "deepspeech2"
    head: str = "ctc"
    dropout: float = 0.0
    chunk_size: int = None
    history_size: int = None
    time_masking: dict = None
    freq_masking: dict = None
    head_size: int = 64   # (no attention: the values only keep ParamStore's head / filter padding off)
    num_heads: int = 1
    filters: int = 64

    def __post_init__(self):
        self.conv_kernels = [[int(v) for v in k] for k in self.conv_kernels]
        self.conv_strides = [[int(v) for v in k] for k in self.conv_strides]
        self.conv_filters = [int(v) for v in self.conv_filters]
        if not len(self.conv_kernels) == len(self.conv_strides) == len(self.conv_filters) >= 1:  # encoders/deepspeech2.py:160
            raise ValueError("conv_kernels, conv_strides and conv_filters must have one entry per block")
        if self.conv_type != "conv2d":
            raise NotImplementedError(f"conv_type={self.conv_type!r}: only conv2d is built")
        if self.rnn_type != "lstm":
            raise NotImplementedError(f"rnn_type={self.rnn_type!r}: only lstm is built (no GRU / SimpleRNN recurrence)")
        for k in ("conv_activation", "fc_activation") + (("rnn_rowconv_activation",) if self.has_rowconv else ()):
            if str(getattr(self, k)) != "relu":
                raise NotImplementedError(f"{k}={getattr(self, k)!r}: only relu is built")
        if self.conv_padding not in ("same", "causal"):
            raise NotImplementedError(f"conv_padding={self.conv_padding!r}: 'same' or 'causal'")
        if self.feature_type not in ("log_mel_spectrogram", "spectrogram"):
            raise NotImplementedError(f"feature_type={self.feature_type!r}: 'log_mel_spectrogram' or 'spectrogram'")
        if self.feature_type == "spectrogram" and not 1 <= int(self.num_feature_bins) <= self.nfft // 2 + 1:
            raise NotImplementedError(f"num_feature_bins={self.num_feature_bins}: a spectrogram has at most nfft / 2 + 1 bins")
        cin = 1
        for (kh, kw), (st, sf), co in zip(self.conv_kernels, self.conv_strides, self.conv_filters):
            if not (1 <= kh <= 16 and 1 <= kw <= 48 and st in (1, 2, 3) and sf in (1, 2) and (cin == 1 or (cin % 16 == 0 and cin <= 128))
                    and co % 16 == 0 and 16 <= co <= 128):
                raise NotImplementedError(f"conv block kernel {[kh, kw]} strides {[st, sf]} channels {cin}->{co}: the Conv2D kernel takes up to "
                                          "16 x 48 taps, strides (1..3, 1..2), 1 or a multiple of 16 (<= 128) input channels and a multiple "
                                          "of 16 (<= 128) filters")
            cin = co
        if int(self.rnn_nlayers) < 1 or int(self.rnn_units) < 1 or int(self.rnn_units) % 16:
            raise NotImplementedError(f"rnn_nlayers={self.rnn_nlayers} rnn_units={self.rnn_units}: at least one layer, units a multiple of 16")
        if self.has_rowconv and 2 * int(self.rnn_rowconv) + 1 > 32:
            raise NotImplementedError(f"rnn_rowconv={self.rnn_rowconv}: the depthwise kernel takes up to 32 taps")
        if int(self.fc_nlayers) > 0 and int(self.fc_units) % 16:
            raise NotImplementedError(f"fc_units={self.fc_units}: a multiple of 16")

    @property
    def has_rowconv(self):
        """encoders/deepspeech2.py:231: RowConv1D only behind a unidirectional recurrence (rnn_rowconv is ignored otherwise)"""
        return (not self.rnn_bidirectional) and int(self.rnn_rowconv) > 0

    @property
    def ndir(self):
        return 2 if self.rnn_bidirectional else 1

    @property
    def rnn_out(self):
        return self.ndir * int(self.rnn_units)

    @property
    def dmodel(self):
        return int(self.fc_units) if int(self.fc_nlayers) > 0 else self.rnn_out

    @property
    def frame_length(self):
        return int(round(self.sample_rate * self.frame_ms / 1000.0))

    @property
    def frame_step(self):
        return int(round(self.sample_rate * self.stride_ms / 1000.0))

    @property
    def time_reduction_factor(self):
        """encoders/deepspeech2.py:165-181: the product of the blocks' time strides"""
        f = 1
        for st, _ in self.conv_strides:
            f *= st
        return f

    def conv_shapes(self):
        """[(kh, kw, cin, cout, st, sf, F_in, F_out)] of the conv blocks, F_out = ceil(F_in / sf) under both padding rules"""
        out, cin, F = [], 1, int(self.num_feature_bins)
        for (kh, kw), (st, sf), co in zip(self.conv_kernels, self.conv_strides, self.conv_filters):
            out.append((kh, kw, cin, co, st, sf, F, -(-F // sf)))
            cin, F = co, -(-F // sf)
        return out

    @property
    def rnn_in(self):
        """width of the Reshape behind the conv module (merge_two_last_dims: F' * C)"""
        s = self.conv_shapes()[-1]
        return s[7] * s[3]

    def encoder_length(self, n):
        """ConvBlock.call (:110-116): math_util.conv_output_length per block over the TIME stride - ceil(n / st) under both padding rules"""
        n = int(n)
        for st, _ in self.conv_strides:
            n = -(-n // st)
        return n


_DS2_YAML = dict(num_feature_bins=160, feature_type="spectrogram", conv_kernels=[[11, 41], [11, 21]], conv_strides=[[2, 2], [1, 2]],
                 conv_filters=[32, 32], conv_initializer="he_uniform", rnn_nlayers=5, rnn_units=512, fc_nlayers=1, fc_units=1024,
                 fc_initializer="he_uniform", l2=0.0005, bias_l2=0.0005,
                 time_masking=dict(prob=1.0, num_masks=5, mask_factor=-1, p_upperbound=0.05, mask_value=0),
                 freq_masking=dict(prob=1.0, num_masks=1, mask_factor=27, mask_value=0))


def deepspeech2(vocab_size=1000, variant="base", **over):
    """examples/models/ctc/deepspeech2/base.yml.j2 (2 conv blocks "same", 5 x BiLSTM(512), FC 1024); variant="uni": uni.yml.j2 (causal
    convolutions, 5 x LSTM(512) each followed by RowConv1D(3))."""
    kw = dict(_DS2_YAML, vocab_size=vocab_size)
    if variant == "base":
        kw.update(conv_padding="same", rnn_bidirectional=True, rnn_rowconv=0, rnn_dropout=0.5, fc_dropout=0.5)
    elif variant == "uni":
        kw.update(conv_padding="causal", rnn_bidirectional=False, rnn_rowconv=3, rnn_dropout=0.1, fc_dropout=0.1)
    else:
        raise ValueError(f"variant {variant!r}: 'base' or 'uni'")
    kw.update(over)
    return DeepSpeech2Config(**kw)


def deepspeech2_tiny(vocab_size=29, **over):
    kw = dict(vocab_size=vocab_size, num_feature_bins=16, feature_type="spectrogram", conv_kernels=[[5, 7], [3, 5]], conv_strides=[[2, 2], [1, 2]],
              conv_filters=[16, 16], conv_padding="same", rnn_nlayers=2, rnn_units=32, rnn_bidirectional=True, rnn_rowconv=0, fc_nlayers=1,
              fc_units=64, rnn_dropout=0.0, fc_dropout=0.0)
    kw.update(over)
    return DeepSpeech2Config(**kw)


def deepspeech2_from_reference(config: dict):
    """The YAML's `model_config.config` of tensorflow_asr.models.ctc.deepspeech2>DeepSpeech2 (base.yml.j2:3-54) -> DeepSpeech2Config.
    Options that are not built raise with the option named (DeepSpeech2Config.__post_init__, speech_kwargs); rnn_unroll changes nothing
    in the reference's arithmetic and is accepted either way."""
    c = dict(config)
    sc = dict(c.get("speech_config", {}))
    aug = (sc.get("augmentation_config") or {}).get("feature_augment", {}) or {}

    def _l2(reg, key):
        if reg is None:
            return 0.0
        if not isinstance(reg, dict) or str(reg.get("class_name", "l2")).lower() != "l2":
            raise NotImplementedError(f"{key}={reg!r}: only an l2 regulariser is known")
        return float((reg.get("config") or {}).get("l2", 0.0))

    kw = dict(**speech_kwargs(sc, feature_types=("log_mel_spectrogram", "spectrogram")), feature_type=str(sc.get("feature_type", "log_mel_spectrogram")),
              l2=_l2(c.get("kernel_regularizer"), "kernel_regularizer"), bias_l2=_l2(c.get("bias_regularizer"), "bias_regularizer"))
    if c.get("activity_regularizer") is not None:
        raise NotImplementedError(f"activity_regularizer={c['activity_regularizer']!r}: not built")
    fields = {f for f in DeepSpeech2Config.__dataclass_fields__}
    for k, v in c.items():
        if k in ("speech_config", "kernel_regularizer", "bias_regularizer", "activity_regularizer", "name"):
            continue
        if k not in fields or k in ("encoder", "head", "head_size", "num_heads", "filters", "chunk_size", "history_size", "dropout", "l2", "bias_l2",
                                     "feature_type", "time_masking", "freq_masking"):
            raise NotImplementedError(f"{k}={v!r}: not a keyword of models/ctc/deepspeech2.py:58-89 that is built here")
        kw[k] = v
    if "time_masking" in aug:
        kw["time_masking"] = dict(aug["time_masking"])
    if "freq_masking" in aug:
        kw["freq_masking"] = dict(aug["freq_masking"])
    return DeepSpeech2Config(**kw)


# ------------------------------------------------------------------------------------------------------------------ Transformer (CTC / transducer)
@dataclass
class TransformerConfig:
    """The keyword surface of tensorflow_asr.models.ctc.transformer.Transformer (models/ctc/transformer.py:56-87) and
    tensorflow_asr.models.transducer.transformer.Transformer (models/transducer/transformer.py:21-67) with `speech_config` flattened as in
    ConformerConfig and the `encoder_` prefix dropped.  The defaults are the shipped examples/models/ctc/transformer/base.yml.j2 (which says
    `mha`; the classes' own default `relmha` is not built).  Inference only: the dropout rate is kept for the record and never applied."""
    # speech_config
    sample_rate: int = 16000
    frame_ms: int = 25
    stride_ms: int = 10
    nfft: int = 512
    num_feature_bins: int = 80
    preemphasis: float = 0.97
    epsilon: float = 1e-6
    lower_edge_hertz: float = 0.0
    upper_edge_hertz: float = 8000.0
    # encoder (models/encoders/transformer.py:196-222)
    sub_filters: list = field(default_factory=lambda: [512, 512])   # encoder_subsampling.filters (conv2d, 3x3 stride-2 causal blocks, relu)
    sub_norm: str = "batch"                                         # encoder_subsampling.norms: both "batch" or both "none"
    dmodel: int = 512
    dff: int = 1024
    num_blocks: int = 6
    head_size: int = 128
    num_heads: int = 4
    mha_type: str = "mha"
    interleave_relpe: bool = True
    use_attention_causal_mask: bool = False
    use_attention_auto_mask: bool = True
    residual_factor: float = 1.0
    norm_position: str = "post"
    pwffn_activation: str = "relu"
    dropout: float = 0.1
    chunk_size: int = None
    history_size: int = None
    # model head: "ctc" (TransformerDecoder: one Dense(vocab) "logits") or "transducer" (prediction + joint networks, base_transducer.py)
    head: str = "ctc"
    embed_dim: int = 512
    rnn_units: int = 320
    joint_dim: int = 1024
    prediction_layer_norm: bool = True
    vocab_size: int = 1000
    blank: int = 0
    l2: float = 1e-6
    # what the shared model code reads from every config
    encoder: str = "transformer"
    time_masking: dict = None
    freq_masking: dict = None

    def __post_init__(self):
        self.sub_filters = [int(v) for v in self.sub_filters]
        if len(self.sub_filters) != 2 or any(c <= 0 or c % 8 for c in self.sub_filters):
            raise NotImplementedError(f"encoder_subsampling.filters={self.sub_filters}: two 3x3 stride-2 blocks, filters a multiple of 8")
        if self.sub_norm not in ("batch", "none"):
            raise NotImplementedError(f"encoder_subsampling.norms={self.sub_norm!r}: 'batch' or 'none'")
        if self.mha_type != "mha":
            raise NotImplementedError(f"encoder_mha_type={self.mha_type!r}: only mha (plain attention over absolute positions) is built in this encoder")
        if self.norm_position not in ("post", "pre"):
            raise NotImplementedError(f"encoder_norm_position={self.norm_position!r}: 'post' or 'pre'")
        if self.pwffn_activation != "relu":
            raise NotImplementedError(f"encoder_pwffn_activation={self.pwffn_activation!r}: only relu is built")
        if self.head not in ("ctc", "transducer"):
            raise ValueError(f"head {self.head!r}: 'ctc' or 'transducer'")
        if (self.chunk_size is None) != (self.history_size is None):  # multihead_attention.py:342 needs both
            self.chunk_size = self.history_size = None
        if self.chunk_size is not None and int(self.chunk_size) < 1:
            raise ValueError("encoder_chunk_size must be positive")
        d, dh, dff = int(self.dmodel), int(self.head_size), int(self.dff)
        if dh % 16 or dh > 128 or dh < 16:
            raise NotImplementedError(f"encoder_head_size={dh}: the plain-attention kernels take a multiple of 16 up to 128 (64 | 128 in bf16)")
        if d % 16 or dff % 16 or d < 16:
            raise NotImplementedError(f"encoder_dmodel={d} encoder_dff={dff}: multiples of 16")
        if int(self.num_blocks) < 1 or int(self.num_heads) < 1:
            raise ValueError("encoder_num_blocks and encoder_num_heads must be positive")

    @property
    def filters(self):  # (ParamStore's filter padding reads it; nothing is padded here)
        return self.sub_filters[0]

    @property
    def sub_freq(self):
        """frequency bins behind the two stride-2 blocks"""
        return -(-(-(-int(self.num_feature_bins) // 2)) // 2)

    @property
    def frame_length(self):
        return int(round(self.sample_rate * self.frame_ms / 1000.0))

    @property
    def frame_step(self):
        return int(round(self.sample_rate * self.stride_ms / 1000.0))

    @property
    def time_reduction_factor(self):
        return 4

    def encoder_length(self, n):
        """Conv2dSubsampling.call (subsampling.py:218-230): math_util.conv_output_length "causal" per block = ceil(n / 2) twice"""
        return -(-(-(-int(n) // 2)) // 2)


def transformer(vocab_size=1000, head="ctc", streaming=False, **over):
    """examples/models/ctc/transformer/base.yml.j2 (d 512, 6 blocks, 4 heads of 128, dff 1024, post-norm, mha); streaming=True:
    base-streaming.yml.j2 (chunk 16, history 64).  head="rnnt": the same encoder under the transducer class with its constructor's
    prediction / joint defaults (models/transducer/transformer.py:45-60; the reference ships no YAML for it)."""
    if head not in ("ctc", "rnnt", "transducer"):
        raise ValueError(f"head {head!r}: 'ctc' or 'rnnt'")
    kw = dict(vocab_size=vocab_size, head="ctc" if head == "ctc" else "transducer",
              time_masking=dict(prob=1.0, num_masks=5, mask_factor=-1, p_upperbound=0.05), freq_masking=dict(prob=1.0, num_masks=2, mask_factor=27))
    if streaming:
        kw.update(chunk_size=16, history_size=64)
    kw.update(over)
    return TransformerConfig(**kw)


def transformer_tiny(vocab_size=29, head="ctc", **over):
    kw = dict(vocab_size=vocab_size, head="ctc" if head == "ctc" else "transducer", num_feature_bins=16, sub_filters=[16, 16], dmodel=64, dff=128,
              num_blocks=2, head_size=64, num_heads=2, dropout=0.0, embed_dim=24, rnn_units=24, joint_dim=40)
    kw.update(over)
    return TransformerConfig(**kw)


_TRANSFORMER_KEYS = {  # constructor keyword -> field, of both reference classes
    "encoder_dmodel": "dmodel", "encoder_dff": "dff", "encoder_num_blocks": "num_blocks", "encoder_head_size": "head_size",
    "encoder_num_heads": "num_heads", "encoder_mha_type": "mha_type", "encoder_interleave_relpe": "interleave_relpe",
    "encoder_use_attention_causal_mask": "use_attention_causal_mask", "encoder_use_attention_auto_mask": "use_attention_auto_mask",
    "encoder_residual_factor": "residual_factor", "encoder_norm_position": "norm_position", "encoder_pwffn_activation": "pwffn_activation",
    "encoder_dropout": "dropout", "encoder_history_size": "history_size", "encoder_chunk_size": "chunk_size",
    "prediction_embed_dim": "embed_dim", "prediction_rnn_units": "rnn_units", "prediction_layer_norm": "prediction_layer_norm",
    "joint_dim": "joint_dim", "vocab_size": "vocab_size", "blank": "blank",
}
_TRANSFORMER_ONLY = {  # keywords that change the network and are built for one value only
    "encoder_memory_length": (None,), "encoder_trainable": (True,), "decoder_trainable": (True,), "bias_regularizer": (None,),
    "activity_regularizer": (None,), "prediction_label_encode_mode": ("embedding",), "prediction_num_rnns": (1,),
    "prediction_rnn_type": ("lstm",), "prediction_projection_units": (0,), "prediction_trainable": (True,), "joint_activation": ("tanh",),
    "prejoint_encoder_linear": (True,), "prejoint_prediction_linear": (True,), "postjoint_linear": (False,), "joint_mode": ("add",),
    "joint_trainable": (True,),
}
_TRANSFORMER_IGNORED = ("name", "speech_config", "encoder_subsampling", "kernel_regularizer",
                        # change nothing in the inference arithmetic of the mha encoder: relmha's own causal switch, the attention
                        # implementation hint, keras' LSTM implementation / unroll switches
                        "encoder_mha_causal", "encoder_flash_attention", "prediction_rnn_implementation", "prediction_rnn_unroll")


def transformer_from_reference(config: dict, head="ctc", class_name: str = None):
    """The YAML's `model_config.config` of tensorflow_asr.models.ctc.transformer>Transformer (base.yml.j2:3-50) or of the transducer class
    -> TransformerConfig.  A keyword the mapping omits takes the CLASS's default (so an mha model must say `encoder_mha_type: mha`, as the
    shipped files do).  Every keyword is mapped or raises NotImplementedError with its name."""
    c = dict(config)
    if class_name is not None:
        head = "ctc" if ".ctc." in class_name else "rnnt"
    if head not in ("ctc", "rnnt", "transducer"):
        raise ValueError(f"head {head!r}: 'ctc' or 'rnnt'")
    ctc = head == "ctc"
    sc = dict(c.get("speech_config", {}))
    aug = (sc.get("augmentation_config") or {}).get("feature_augment", {}) or {}
    for k, ok in _TRANSFORMER_ONLY.items():
        if k in c and c[k] not in ok:
            raise NotImplementedError(f"{k}={c[k]!r}: only {ok} is built")
    if not ctc and "prediction_layer_norm" in c and not c["prediction_layer_norm"]:
        raise NotImplementedError("prediction_layer_norm=False: the transducer's prediction network ends in a LayerNorm here")
    sub = dict(c.get("encoder_subsampling") or {})
    stype = sub.pop("type", None)
    if stype != "conv2d":
        raise NotImplementedError(f"encoder_subsampling.type={stype!r}: only conv2d is built (not vgg / conv1d)")
    if "filters" not in sub:
        raise ValueError("encoder_subsampling.filters is required (subsampling.py:166)")

    def _pairs(v):
        return [list(x) if isinstance(x, (list, tuple)) else [x, x] for x in v]

    # keys the mapping omits take Conv2dSubsampling's own defaults (subsampling.py:166-171)
    kernels, strides = _pairs(sub.pop("kernels", [[3, 3], [3, 3]])), _pairs(sub.pop("strides", [[2, 1], [2, 1]]))
    paddings, norms = [str(v) for v in sub.pop("paddings", ["causal", "causal"])], [str(v) for v in sub.pop("norms", ["none", "none"])]
    acts = [str(v) for v in sub.pop("activations", ["relu", "relu"])]
    filters = list(sub.pop("filters"))
    if sub:
        raise NotImplementedError(f"encoder_subsampling.{sorted(sub)[0]}: not a keyword of Conv2dSubsampling")
    if kernels != [[3, 3], [3, 3]] or strides != [[2, 2], [2, 2]]:
        raise NotImplementedError(f"encoder_subsampling kernels={kernels} strides={strides}: only two 3x3 stride-2 blocks are built")
    if paddings != ["causal", "causal"]:
        raise NotImplementedError(f"encoder_subsampling.paddings={paddings}: only causal")
    if norms not in (["batch", "batch"], ["none", "none"]):
        raise NotImplementedError(f"encoder_subsampling.norms={norms}: both 'batch' or both 'none'")
    if acts != ["relu", "relu"]:
        raise NotImplementedError(f"encoder_subsampling.activations={acts}: only relu")
    reg = c.get("kernel_regularizer") or {}
    if reg and (not isinstance(reg, dict) or str(reg.get("class_name", "l2")).lower() != "l2"):
        raise NotImplementedError(f"kernel_regularizer={reg!r}: only an l2 regulariser is known")
    kw = dict(**speech_kwargs(sc), sub_filters=filters, sub_norm=norms[0], head="ctc" if ctc else "transducer", mha_type="relmha",
              l2=float((reg.get("config") or {}).get("l2", 0.0)) if reg else 0.0)
    for k, v in c.items():
        if k in _TRANSFORMER_IGNORED or k in _TRANSFORMER_ONLY:
            continue
        if k not in _TRANSFORMER_KEYS or (ctc and k.startswith(("prediction_", "joint_"))):
            raise NotImplementedError(f"{k}={v!r}: not a keyword of the reference's Transformer class that is built here")
        kw[_TRANSFORMER_KEYS[k]] = v
    if "time_masking" in aug:
        kw["time_masking"] = dict(aug["time_masking"])
    if "freq_masking" in aug:
        kw["freq_masking"] = dict(aug["freq_masking"])
    return TransformerConfig(**kw)


def transformer_schedule(step, dmodel, warmup_steps=10000, scale=2.0, max_lr=None, min_lr=None):
    """TransformerSchedule.__call__ (optimizers/schedules.py:28-37)."""
    step = float(step)
    # step 0 (keras' `iterations` at the first update): tf gives min(inf, 0) = 0
    lr = scale * dmodel ** -0.5 * min(step ** -0.5, step * warmup_steps ** -1.5) if step > 0 else 0.0
    if max_lr is not None:
        lr = min(max_lr, lr)
    if min_lr is not None:
        lr = max(min_lr, lr)
    return lr


# ------------------------------------------------------------------------------------------------------------------ RNN-Transducer
@dataclass
class RnnTransducerConfig:
    """The keyword surface of tensorflow_asr.models.transducer.rnnt.RnnTransducer (models/transducer/rnnt.py:23-59) with `speech_config`
    flattened as in ConformerConfig and the `encoder_` prefix dropped where no prediction keyword of the same name exists.  The defaults
    are the shipped examples/models/transducer/rnnt/small.yml.j2 (the class's own defaults - two prediction LSTMs with a projection - are
    not built).  Inference only: the regulariser is kept for the record and never applied."""
    # speech_config
    sample_rate: int = 16000
    frame_ms: int = 25
    stride_ms: int = 10
    nfft: int = 512
    num_feature_bins: int = 80
    preemphasis: float = 0.97
    epsilon: float = 1e-6
    lower_edge_hertz: float = 0.0
    upper_edge_hertz: float = 8000.0
    # encoder (models/encoders/rnnt.py:131-146)
    reduction_positions: list = field(default_factory=lambda: ["post", "post", "post", "post"])
    reduction_factors: list = field(default_factory=lambda: [3, 0, 2, 0])
    encoder_dmodel: int = 320   # the blocks' Dense "projection" width; `dmodel` below is the width of the encoder's OUTPUT rows
    nlayers: int = 4
    encoder_rnn_type: str = "lstm"
    encoder_rnn_units: int = 1024
    layer_norm: bool = True   # encoder_layer_norm
    # prediction / joint (base_transducer.py), the names the shared head reads
    embed_dim: int = 512
    rnn_units: int = 1024     # prediction_rnn_units
    joint_dim: int = 320
    prediction_layer_norm: bool = True
    vocab_size: int = 1000
    blank: int = 0
    l2: float = 1e-6
    # what the shared model code reads from every config
    encoder: str = "rnnt"
    head: str = "transducer"
    dropout: float = 0.0
    chunk_size: int = None
    history_size: int = None
    time_masking: dict = None
    freq_masking: dict = None
    head_size: int = 64   # (no attention, no convolution: the values only keep ParamStore's head / filter padding off)
    num_heads: int = 1
    filters: int = 64

    def __post_init__(self):
        self.reduction_positions = [str(p) for p in self.reduction_positions]
        self.reduction_factors = [int(f) for f in self.reduction_factors]
        self.nlayers = int(self.nlayers)
        if self.nlayers < 1:
            raise ValueError("encoder_nlayers must be positive")
        if len(self.reduction_positions) != self.nlayers:  # encoders/rnnt.py:147-148
            raise ValueError("encoder_reduction_positions length must be equal to encoder_nlayers")
        if len(self.reduction_factors) != self.nlayers:
            raise ValueError("encoder_reduction_factors length must be equal to encoder_nlayers")
        if any(p not in ("pre", "post") for p in self.reduction_positions):  # encoders/rnnt.py:43
            raise ValueError("encoder_reduction_positions: every entry must be 'post' or 'pre'")
        if any(f < 0 for f in self.reduction_factors):
            raise ValueError("encoder_reduction_factors: every entry must be >= 0 (0: no reduction)")
        if self.encoder_rnn_type != "lstm":
            raise NotImplementedError(f"encoder_rnn_type={self.encoder_rnn_type!r}: only lstm is built (no GRU / SimpleRNN recurrence)")
        if int(self.encoder_rnn_units) < 32 or int(self.encoder_rnn_units) % 32:
            raise NotImplementedError(f"encoder_rnn_units={self.encoder_rnn_units}: a multiple of 32")
        if int(self.encoder_dmodel) < 16 or int(self.encoder_dmodel) % 16:
            raise NotImplementedError(f"encoder_dmodel={self.encoder_dmodel}: a multiple of 16")
        for i, f in enumerate(self.factors):
            if (self.block_in(i) * (f if self.reduction_positions[i] == "pre" else 1)) % 8:
                raise NotImplementedError(f"block {i}: an LSTM input width of {self.block_in(i)} x {f} is not a multiple of 8")

    @property
    def factors(self):
        """the blocks' effective reduction factors (0 = no TimeReduction layer = 1)"""
        return [max(int(f), 1) for f in self.reduction_factors]

    def block_in(self, i):
        """width of block i's input rows in front of its own `pre` reduction"""
        if i == 0:
            return int(self.num_feature_bins)
        return int(self.encoder_dmodel) * (self.factors[i - 1] if self.reduction_positions[i - 1] == "post" else 1)

    def lstm_in(self, i):
        return self.block_in(i) * (self.factors[i] if self.reduction_positions[i] == "pre" else 1)

    @property
    def dmodel(self):
        """width of the encoder's output rows (what the joint network's encoder projection is built on): a `post` reduction of the LAST
        block folds its factor into them"""
        return int(self.encoder_dmodel) * (self.factors[-1] if self.reduction_positions[-1] == "post" else 1)

    @property
    def frame_length(self):
        return int(round(self.sample_rate * self.frame_ms / 1000.0))

    @property
    def frame_step(self):
        return int(round(self.sample_rate * self.stride_ms / 1000.0))

    @property
    def time_reduction_factor(self):
        """encoders/rnnt.py:153-169: the product of the blocks' factors"""
        return int(math.prod(self.factors))

    def encoder_length(self, n):
        """math_util.get_reduced_length layer by layer (subsampling.py:39): ceil(n / f) per reducing block"""
        n = int(n)
        for f in self.factors:
            n = -(-n // f)
        return n


def rnnt(vocab_size=1000, **over):
    """examples/models/transducer/rnnt/small.yml.j2: 4 x (LSTM(1024) -> LayerNorm -> Dense(320)), `post` reductions 3 and 2."""
    kw = dict(vocab_size=vocab_size, time_masking=dict(prob=1.0, num_masks=5, mask_factor=-1, p_upperbound=0.05),
              freq_masking=dict(prob=1.0, num_masks=1, mask_factor=27))
    kw.update(over)
    return RnnTransducerConfig(**kw)


def rnnt_tiny(vocab_size=29, **over):
    kw = dict(vocab_size=vocab_size, num_feature_bins=16, reduction_positions=["post", "post", "pre"], reduction_factors=[3, 0, 2], encoder_dmodel=16,
              nlayers=3, encoder_rnn_units=32, embed_dim=24, rnn_units=24, joint_dim=40)
    kw.update(over)
    return RnnTransducerConfig(**kw)


_RNNT_KEYS = {  # constructor keyword -> field (models/transducer/rnnt.py:23-59)
    "encoder_reduction_positions": "reduction_positions", "encoder_reduction_factors": "reduction_factors", "encoder_dmodel": "encoder_dmodel",
    "encoder_nlayers": "nlayers", "encoder_rnn_type": "encoder_rnn_type", "encoder_rnn_units": "encoder_rnn_units",
    "encoder_layer_norm": "layer_norm", "prediction_embed_dim": "embed_dim", "prediction_rnn_units": "rnn_units",
    "prediction_layer_norm": "prediction_layer_norm", "joint_dim": "joint_dim", "vocab_size": "vocab_size", "blank": "blank",
}
_RNNT_CLASS_DEFAULTS = {  # what the class takes for a keyword the mapping omits (rnnt.py:28-52)
    "encoder_reduction_positions": ["pre"] * 8, "encoder_reduction_factors": [6, 0, 0, 0, 0, 0, 0, 0], "encoder_dmodel": 640,
    "encoder_nlayers": 8, "encoder_rnn_type": "lstm", "encoder_rnn_units": 2048, "encoder_layer_norm": False, "prediction_embed_dim": 320,
    "prediction_rnn_units": 2048, "prediction_layer_norm": False, "joint_dim": 640,
    "prediction_label_encode_mode": "embedding", "prediction_num_rnns": 2, "prediction_rnn_type": "lstm", "prediction_projection_units": 640,
    "joint_activation": "tanh", "prejoint_encoder_linear": True, "prejoint_prediction_linear": True, "postjoint_linear": False,
    "joint_mode": "add",
}
_RNNT_ONLY = {  # keywords that change the network and are built for one value only (the head is ConformerTransducer's)
    "encoder_trainable": (True,), "prediction_trainable": (True,), "joint_trainable": (True,), "bias_regularizer": (None,),
    "activity_regularizer": (None,), "prediction_label_encode_mode": ("embedding",), "prediction_num_rnns": (1,),
    "prediction_rnn_type": ("lstm",), "prediction_projection_units": (0,), "prediction_layer_norm": (True,), "joint_activation": ("tanh",),
    "prejoint_encoder_linear": (True,), "prejoint_prediction_linear": (True,), "postjoint_linear": (False,), "joint_mode": ("add",),
}
_RNNT_IGNORED = ("name", "speech_config", "kernel_regularizer",
                 # keras' LSTM implementation / unroll switches change nothing in the inference arithmetic
                 "encoder_rnn_unroll", "prediction_rnn_implementation", "prediction_rnn_unroll")


def rnnt_from_reference(config: dict):
    """The YAML's `model_config.config` of tensorflow_asr.models.transducer.rnnt>RnnTransducer (small.yml.j2:3-49) -> RnnTransducerConfig.
    A keyword the mapping omits takes the CLASS's default - so a mapping must say `prediction_num_rnns: 1`, `prediction_projection_units:
    0` and `prediction_layer_norm: True`, as the shipped file does.  Every keyword is mapped or raises NotImplementedError with its name."""
    c = dict(_RNNT_CLASS_DEFAULTS)
    c.update(config)
    sc = dict(c.get("speech_config") or {})
    aug = (sc.get("augmentation_config") or {}).get("feature_augment", {}) or {}
    for k, ok in _RNNT_ONLY.items():
        if k in c and c[k] not in ok:
            raise NotImplementedError(f"{k}={c[k]!r}: only {ok} is built")
    reg = c.get("kernel_regularizer") or {}
    if reg and (not isinstance(reg, dict) or str(reg.get("class_name", "l2")).lower() != "l2"):
        raise NotImplementedError(f"kernel_regularizer={reg!r}: only an l2 regulariser is known")
    kw = dict(**speech_kwargs(sc), l2=float((reg.get("config") or {}).get("l2", 0.0)) if reg else 0.0)
    for k, v in c.items():
        if k in _RNNT_IGNORED or (k in _RNNT_ONLY and k not in _RNNT_KEYS):
            continue
        if k not in _RNNT_KEYS:
            raise NotImplementedError(f"{k}={v!r}: not a keyword of models/transducer/rnnt.py:23-59 that is built here")
        kw[_RNNT_KEYS[k]] = v
    if "time_masking" in aug:
        kw["time_masking"] = dict(aug["time_masking"])
    if "freq_masking" in aug:
        kw["freq_masking"] = dict(aug["freq_masking"])
    return RnnTransducerConfig(**kw)
