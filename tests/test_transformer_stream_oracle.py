"""The chunk-by-chunk Transformer oracle (tests/transformer_stream_oracle.py) against the offline float64 oracle
(tests/transformer_oracle.py), without a GPU: an utterance run alone, cut at any feature frame, gives in its completed chunks exactly
the offline frames - and why the contract has to say "alone"."""
import numpy as np
import pytest
import torch

import transformer_cases as C
import transformer_oracle as TO
import transformer_stream_oracle as TSO

CASES = {"chunked": {}, "causal": dict(use_attention_causal_mask=True), "pre": dict(norm_position="pre")}
_CACHE = {}


def case(name):
    """config, weights, the features of each utterance ALONE (its own samples and nothing behind them), the padded batch's features, and
    the offline oracle of each utterance alone; computed once"""
    if name not in _CACHE:
        cfg = C.tiny_config("chunked", **CASES[name])
        W = C.make_weights(cfg)
        sig = C.audio()
        flen = [-(-n // cfg.frame_step) for n in C.SAMPLES]
        own = [C.features(sig[b:b + 1, :n], cfg)[0] for b, n in enumerate(C.SAMPLES)]
        assert [f.shape[0] for f in own] == flen
        alone = [TSO.offline_alone(f, W, cfg) for f in own]
        _CACHE[name] = dict(cfg=cfg, W=W, own=own, batch=C.features(sig, cfg), flen=flen, alone=alone)
    return _CACHE[name]


def _maxabs(a, b):
    return float((a - b).abs().max())


@pytest.mark.parametrize("name", list(CASES))
def test_chunked_oracle_equals_the_offline_oracle_alone_at_every_arrival_granularity(name):
    """from one feature frame per call to the whole utterance in one call; utterance 1 (13 encoder frames) ends in a partial chunk and
    utterance 0 (31 feature frames) in a chunk that is full only after the rounding up of the two stride-2 blocks"""
    c = case(name)
    assert (c["cfg"].chunk_size, c["cfg"].history_size) == (4, 8)
    worst = 0.0
    for b in range(3):
        feat, want = c["own"][b], c["alone"][b]
        assert want.shape[0] == C.ELEN[b]
        for per_call in range(1, feat.shape[0] + 1):
            got = TSO.stream_encoder(feat, per_call, c["W"], c["cfg"])
            assert got.shape == want.shape, (b, per_call)
            worst = max(worst, _maxabs(got, want))
    print(f"{name}: chunked against offline alone, every granularity: max abs {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", list(CASES))
def test_a_truncated_utterance_agrees_on_its_completed_chunks(name):
    """the utterance cut after any number of feature frames: the frames of the chunks that are complete at the cut do not change when
    the rest arrives (nothing looks ahead past a chunk)"""
    c = case(name)
    feat, whole = c["own"][2], c["alone"][2]
    n0 = 4 * c["cfg"].chunk_size
    for cut in range(1, feat.shape[0] + 1):
        done = (cut // n0) * c["cfg"].chunk_size
        if done:
            got = TSO.offline_alone(feat[:cut], c["W"], c["cfg"])
            assert _maxabs(got[:done], whole[:done]) <= 1e-12, cut


def test_a_batch_row_is_the_utterance_alone_only_where_no_padded_frame_is_a_visible_key():
    """rows 0 (T' = 8: whole chunks) and 2 (the longest) of the padded batch are the utterances alone; row 1 (T' = 13) is not: the
    padded frames 13 .. 15 of its last chunk are keys its valid rows see.  This is why a session promises the utterance ALONE."""
    c = case("chunked")
    enc, lens = TO.encoder(c["batch"], c["flen"], c["cfg"], c["W"])
    assert lens == C.ELEN
    diff = [_maxabs(enc[b, :lens[b]], c["alone"][b]) for b in range(3)]
    print("batch row against the utterance alone:", diff)
    assert diff[0] <= 1e-6 and diff[2] <= 1e-6 and diff[1] > 1e-3


def test_slot_arithmetic_of_the_rings():
    """a ring that wraps, more rows than slots, and no ring at all"""
    rows = torch.arange(40, dtype=torch.float64).view(20, 2)
    ring = torch.zeros(3, 2, dtype=torch.float64)
    seen = 0
    for n in (2, 2, 1, 4, 5, 1):
        TSO.ring_append(ring, rows[seen:seen + n], seen, 3)
        seen += n
        got = TSO.ring_history(ring, seen, 3)
        assert torch.equal(got, rows[max(0, seen - 3):seen]), seen
    empty = torch.zeros(0, 2, dtype=torch.float64)
    TSO.ring_append(empty, rows[:4], 0, 0)
    assert TSO.ring_history(empty, 4, 0).shape[0] == 0
    q = torch.randn(3, 2, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    full = TSO.attn_chunk(q, q, q, q[:0], q[:0], 0.5)
    causal = TSO.attn_chunk(q, q, q, q[:0], q[:0], 0.5, causal=True)
    assert torch.allclose(causal[0], q[0]) and torch.allclose(causal[2], full[2]) and not torch.allclose(causal[1], full[1])
    np.testing.assert_allclose(TSO.attn_chunk(q[:1], q[:1], q[:1], q[1:], q[1:], 0.5).numpy(), full[:1].numpy(), rtol=1e-12)
