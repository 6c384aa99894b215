"""The yardstick of the streaming tests, proven on the CPU: the chunked f64 oracle (tests/stream_oracle.py) equals the offline oracle of
each golden utterance run ALONE, and row 0 (the longest utterance, which the reference's padded batch treats as if alone) equals the
reference-made golden.  These pass without the streaming kernels: the GPU tests compare against something already proven."""
import numpy as np
import pytest
import torch

from oracle import conformer_ref as R

import stream_oracle as SO

GRANULARITIES = (3, 8, 11, 1000)  # feature frames per call (chunk 2 = 8 feature frames: below, equal, above, all at once)


def _close(a, b, tol=2e-5):  # the bar of tests/test_reference_wiring.py
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b).max() / max(1.0, np.abs(b).max())
    assert err < tol, err


def _utts(z):
    return [z["signals"][b, :int(z["signals_length"][b])] for b in range(z["signals"].shape[0])]


@pytest.mark.parametrize("norms", ["layer", "batch"])
def test_chunked_encoder_equals_offline_alone(norms):
    z, W = SO.load_golden()
    over = dict(SO.STREAM_OVER)
    if norms == "batch":  # batch norms on moving statistics: per-frame arithmetic as well (statistics drawn here, the golden has none)
        over.update(convm_dw_norm="batch", sub_norm="batch")
        g = torch.Generator().manual_seed(5)
        for k in [k for k in W if k.endswith("bn/g") or k.endswith("bn0/g") or k.endswith("bn1/g")]:
            base = k[:-2]
            W[base + "/mm"] = torch.randn(W[k].shape, generator=g, dtype=torch.float64) * 0.1
            W[base + "/mv"] = torch.rand(W[k].shape, generator=g, dtype=torch.float64) + 0.5
    cfg = SO.oracle_cfg(**over)
    for sig in _utts(z):
        off, feat = SO.offline_alone(sig, W, cfg)
        for fpc in GRANULARITIES:
            st = SO.stream_encoder(torch.from_numpy(feat), fpc, W, cfg)
            assert st.shape == off.shape
            assert float((st - off).abs().max()) < 1e-12, (fpc, float((st - off).abs().max()))


def test_row0_alone_is_the_reference_made_golden_row():
    z, W = SO.load_golden()
    cfg = SO.oracle_cfg(**SO.STREAM_OVER)
    off, _ = SO.offline_alone(_utts(z)[0], W, cfg)
    T = off.shape[0]
    assert T == int(z["eval/logits_length"][0]) == z["eval/encoder"].shape[1]
    _close(off, z["eval/encoder"][0])
    st = SO.stream_encoder(torch.from_numpy(SO.offline_alone(_utts(z)[0], W, cfg)[1]), 3, W, cfg)
    _close(st, z["eval/encoder"][0])


def test_chunked_logmel_equals_offline():
    z, _ = SO.load_golden()
    cfg = SO.oracle_cfg(**SO.STREAM_OVER)
    for sig in _utts(z):
        off = R.log_mel(sig[None], cfg)[0]
        for piece in (161, 733, 1000, len(sig)):
            got = SO.stream_logmel(sig, piece, cfg)
            assert got.shape == off.shape
            _close(got, off, 1e-5)


def test_search_with_carry_equals_search_on_the_whole():
    z, W = SO.load_golden()
    cfg = SO.oracle_cfg(**SO.STREAM_OVER)
    W = dict(W)
    W["joint/vocab/b"] = W["joint/vocab/b"].clone()
    W["joint/vocab/b"][0] -= 1.0  # (an untrained model prefers the blank: make it speak)
    for sig in _utts(z):
        enc, _ = SO.offline_alone(sig, W, cfg)
        enc = enc[None]
        whole, _, _, _ = R.recognize_single(enc, [enc.shape[1]], W)
        ref, _ = SO.recognize_single_carry(enc, W)
        n = len(ref)
        assert whole[0, :n].tolist() == ref and not whole[0, n:].any()
        for C in (1, 2, 5):
            toks, state = [], None
            for t in range(0, enc.shape[1], C):
                new, state = SO.recognize_single_carry(enc[:, t:t + C], W, state)
                toks += new
            assert toks == ref


def test_ctc_merge_with_carry():
    seq = [0, 3, 3, 0, 3, 4, 4, 4, 0, 0, 5]
    whole, _ = SO.ctc_greedy_carry(seq)
    assert whole == [3, 3, 4, 5]
    for C in (1, 2, 3, 7):
        out, last = [], -1
        for t in range(0, len(seq), C):
            new, last = SO.ctc_greedy_carry(seq[t:t + C], last)
            out += new
        assert out == whole
