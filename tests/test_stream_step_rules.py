"""The step rule of the encoder-stream interface (streaming.EncoderStream.step_rule) for the five encoder kinds, evaluated on the host
without a device: feature frames of a step, encoder rows of a step's output buffer, the frame reduction, and the chunk_frames each
refuses.  The expected values are written out here."""
import pytest

from tensorflowasr_amd import configs, streaming
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.rnnt import RnnTransducer


def _ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("cls,cfg,chunk", [
    (streaming.StreamState, configs.conformer_tiny(chunk_size=4, history_size=8), 4),
    (streaming.TransformerStreamState, configs.transformer_tiny(chunk_size=4, history_size=0), 4),
    (streaming.TransformerStreamState, configs.transformer(streaming=True), 16),
], ids=["conformer_tiny", "transformer_tiny", "transformer_streaming"])
def test_chunked_attention_encoders(cls, cfg, chunk):
    frames, rows, reduce = cls.step_rule(cfg, None)
    assert (frames, rows) == (4 * chunk, chunk)
    assert [reduce(t) for t in range(4 * chunk + 1)] == [_ceil(_ceil(t, 2), 2) for t in range(4 * chunk + 1)]
    assert reduce(frames) == rows
    with pytest.raises(ValueError, match="chunk_frames belongs to"):
        cls.step_rule(cfg, 4 * chunk)


def _strided(cls, cfg):
    factor = int(cfg.time_reduction_factor)
    assert factor > 1
    assert cls.step_rule(cfg, None)[:2] == (32, 32 // factor)
    for n in (factor, 3 * factor, 32 * factor):
        frames, rows, reduce = cls.step_rule(cfg, n)
        assert (frames, rows) == (n, n // factor)
        assert [reduce(t) for t in range(n + 1)] == [_ceil(t, factor) for t in range(n + 1)]
    for bad in (0, factor - 1, factor + 1):
        with pytest.raises(ValueError, match="must be a positive multiple of the time reduction factor"):
            cls.step_rule(cfg, bad)
    return factor


@pytest.mark.parametrize("cfg", [configs.jasper_tiny(), configs.jasper()], ids=["tiny", "base"])
def test_jasper(cfg):
    _strided(streaming.JasperStreamState, cfg)
    assert streaming.JasperStreamState.step_rule(cfg, 4096)[1] == 4096 // int(cfg.time_reduction_factor)  # no row limit


@pytest.mark.parametrize("cfg", [configs.deepspeech2_tiny(conv_padding="causal", rnn_bidirectional=False, rnn_rowconv=2),
                                 configs.deepspeech2(29, variant="uni")], ids=["tiny", "uni"])
def test_deepspeech2(cfg):
    factor = _strided(streaming.DS2StreamState, cfg)
    reduce = streaming.DS2StreamState.step_rule(cfg, factor)[2]
    assert all(reduce(t) == cfg.encoder_length(t) for t in range(200))
    assert streaming.DS2StreamState.step_rule(cfg, factor * K.STREAM_MAX_CHUNK)[1] == K.STREAM_MAX_CHUNK
    with pytest.raises(ValueError, match=f"more than {K.STREAM_MAX_CHUNK} encoder frames a step"):
        streaming.DS2StreamState.step_rule(cfg, factor * (K.STREAM_MAX_CHUNK + 1))


@pytest.mark.parametrize("cfg", [configs.rnnt_tiny(), configs.rnnt()], ids=["tiny", "small"])
def test_rnn_transducer(cfg):
    model = object.__new__(RnnTransducer)  # boundary_factors reads the module list only
    model.cfg = cfg
    model._init_encoder()
    fb = model.boundary_factors()
    assert len(fb) == int(cfg.nlayers) + 1
    for n in (1, 7, 32):
        out_rows = n
        for f in fb:  # in front of every boundary up to f - 1 carried rows join the step's rows; whole groups go on
            out_rows = (f - 1 + out_rows + f - 1) // f if f > 1 else out_rows
        frames, rows, reduce = streaming.RnntStreamState.step_rule(cfg, n)
        assert (frames, rows) == (n, out_rows) and rows >= cfg.encoder_length(n)
        assert all(reduce(t) == cfg.encoder_length(t) for t in range(100))
    assert streaming.RnntStreamState.step_rule(cfg, None)[0] == 32
    with pytest.raises(ValueError, match="must be positive"):
        streaming.RnntStreamState.step_rule(cfg, 0)


def test_dispatch():
    class _M:
        def __init__(self, cfg):
            self.cfg = cfg
            self.ps = type("P", (), dict(head_phys=getattr(cfg, "head_size", 0)))()

    want = {
        "conformer": (streaming.StreamState, configs.conformer_tiny(chunk_size=4, history_size=8)),
        "transformer": (streaming.TransformerStreamState, configs.transformer(streaming=True)),
        "jasper": (streaming.JasperStreamState, configs.jasper_tiny()),
        "deepspeech2": (streaming.DS2StreamState, configs.deepspeech2(29, variant="uni")),
        "rnnt": (streaming.RnntStreamState, configs.rnnt_tiny()),
    }
    assert set(streaming.STREAM_STATES) == set(want)
    for name, (cls, cfg) in want.items():
        assert getattr(cfg, "encoder", "conformer") == name
        assert streaming.STREAM_STATES[name] is cls and streaming.check_streamable(_M(cfg)) is cls
        assert issubclass(cls, streaming.EncoderStream)
    with pytest.raises(ValueError, match="streaming needs a Conformer encoder"):
        streaming.check_streamable(_M(type("C", (), dict(encoder="contextnet"))()))
