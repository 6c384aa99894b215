"""The float64 oracle of the RNN-Transducer encoder (tests/rnnt_oracle.py) held to the recorded run of the reference's own classes
(tests/golden/rnnt_wiring.npz, written by tools/gen_rnnt_fixtures.py), and its chunked walk held to its offline walk.  CPU only.

The fixture is a run that stores float32 between layers: the oracle may differ from it by what the oracle's own arithmetic loses when it
is run in float32 (measured here on the same operands), times 4 for the order of the sums."""
import numpy as np
import pytest

import rnnt_cases as C
import rnnt_oracle as RO


@pytest.fixture(scope="module")
def wiring():
    with np.load(C.WIRING) as z:
        return {k: z[k] for k in z.files}


def _maxerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_offline_walk_matches_the_references_classes(wiring, setting):
    ref = C.reference(setting)
    assert np.array_equal(wiring["feats"], ref["feats"]) and wiring["flen"].tolist() == C.FLEN
    for path, a in checkpoint_arrays(ref).items():  # the fixture's weights are this case's, under the reference's layer names
        assert np.array_equal(wiring[f"{setting}|w|" + path.replace("/", "|")], a), path
    assert wiring[f"{setting}|lengths"].tolist() == ref["elen"] == C.ELEN[setting]
    bar = 4 * _maxerr(ref["enc32"], ref["enc"])
    err = _maxerr(wiring[f"{setting}|encoder"], ref["enc"])  # every row, the padded ones included
    print(f"{setting}: fixture against the f64 oracle {err:.3e} (bar {bar:.3e})")
    assert 0 < bar < 1e-4 and err <= bar


def checkpoint_arrays(ref):
    from tensorflowasr_amd import checkpoint

    return checkpoint.to_keras({k: v for k, v in ref["W"].items() if k.startswith("enc/")}, path_fn=checkpoint.rnnt_keras_path)


def test_call_next_matches_the_references_classes(wiring):
    """two halves with the carried states, [B, nlayers, 2, units]; the second half is ragged (1 / 20 / 50 frames)"""
    ref = C.reference("ln")
    cfg, Wn, feats = ref["cfg"], ref["Wn"], ref["feats"]
    L, P = cfg.nlayers, cfg.encoder_rnn_units
    st = np.zeros((3, L, 2, P))
    bar = 4 * _maxerr(ref["enc32"], ref["enc"])
    for tag, lo, hi in (("1", 0, C.SPLIT), ("2", C.SPLIT, 80)):
        n = [min(max(v - lo, 0), hi - lo) for v in C.FLEN]
        out, lens, st = RO.call_next(feats[:, lo:hi], n, st, cfg, Wn)
        assert wiring["ln|len" + tag].tolist() == lens
        assert wiring["ln|states" + tag].shape == (3, L, 2, P)
        assert _maxerr(wiring["ln|next" + tag], out) <= bar and _maxerr(wiring["ln|states" + tag], st) <= bar, tag
    # the first half is whole groups of 6 for every utterance: its frames are the offline frames
    out1, _, _ = RO.call_next(feats[:, :C.SPLIT], [C.SPLIT] * 3, np.zeros((3, L, 2, P)), cfg, Wn)
    for b in range(3):
        assert _maxerr(out1[b], ref["alone"][b][:C.SPLIT // 6]) < 1e-12


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_a_padded_batch_row_is_not_the_utterance_alone(setting):
    """the reference's behaviour, pinned: in the last reduced frame of a shorter row the group mixes valid frames with rows that are not
    zero (beta W + bias behind a `post` reduction, the features of the padding in front of block 0's `pre` reduction), where the utterance
    alone has tf.pad's zeros.  Every other frame, and the longest row, agree."""
    ref = C.reference(setting)
    f = ref["cfg"].time_reduction_factor
    for b, n in enumerate(ref["elen"]):
        alone, row = ref["alone"][b], ref["enc"][b, :n]
        assert alone.shape[0] == n
        assert _maxerr(alone[:n - 1], row[:n - 1]) < 1e-12
        partial = C.FLEN[b] % f != 0 and C.FLEN[b] != max(C.FLEN)
        if setting == "noln":
            partial = C.FLEN[b] % 2 != 0 and C.FLEN[b] != max(C.FLEN)
        assert (_maxerr(alone[n - 1], row[n - 1]) > 1e-3) == partial, (b, partial)


@pytest.mark.parametrize("setting", list(C.SETTINGS))
@pytest.mark.parametrize("piece", [1, 7, 32, 1000])
def test_chunked_walk_equals_the_offline_walk_alone(setting, piece):
    ref = C.reference(setting)
    for b, n in enumerate(C.FLEN):
        walk = RO.StreamWalk(ref["cfg"], ref["Wn"])
        cuts = list(range(0, n, piece)) + [n]
        got = np.concatenate([walk.step(ref["feats"][b, lo:hi], final=hi == n) for lo, hi in zip(cuts[:-1], cuts[1:])], 0)
        assert got.shape == ref["alone"][b].shape
        assert _maxerr(got, ref["alone"][b]) < 1e-12 and _maxerr(walk.states(), ref["alone_states"][b]) < 1e-12


def test_alone_from_its_own_audio_differs_in_the_last_feature_frames_only():
    """the front end, not the encoder: in a padded batch row the pre-emphasis of the first sample behind the utterance's end reads its last
    sample; the two feature frames that cover it differ from those of the utterance's own audio, and the longest utterance has none"""
    ref = C.reference("ln")
    for b, n in enumerate(C.FLEN):
        d = np.abs(ref["solo_feats"][b][0] - ref["feats"][b, :n]).max(1)
        assert ref["solo_feats"][b].shape == (1, n, 16) and d[:n - 2].max() < 1e-4
        assert (d[n - 2:].max() > 0.1) == (n != max(C.FLEN)), b
        # (chunked from the same features, the walk ends in the states a stream is held to)
        walk = RO.StreamWalk(ref["cfg"], ref["Wn"])
        got = np.concatenate([walk.step(ref["solo_feats"][b][0, lo:lo + 8], final=lo + 8 >= n) for lo in range(0, n, 8)], 0)
        assert _maxerr(got, ref["solo"][b]) < 1e-12 and _maxerr(walk.states(), ref["solo_states"][b]) < 1e-12


def test_boundary_factors_and_lengths():
    cfg = C.tiny_config("ln")
    assert RO.boundary_factors(cfg) == [1, 3, 2, 1] and cfg.time_reduction_factor == 6
    assert RO.boundary_factors(C.tiny_config("noln")) == [2, 1, 1]
    assert [cfg.encoder_length(n) for n in (0, 1, 6, 7, 31, 80)] == [0, 1, 1, 2, 6, 14]
    x = np.arange(2 * 5 * 3, dtype=np.float64).reshape(2, 5, 3)
    y, lens = RO.time_reduction(x, [5, 2], 2)
    assert y.shape == (2, 3, 6) and lens == [3, 1] and not y[:, 2, 3:].any() and np.array_equal(y[0, 0], x[0, :2].reshape(-1))


def test_the_model_speaks():
    for setting in C.SETTINGS:
        ref = C.reference(setting)
        assert all(len(t) > 3 for t in ref["tokens"]) and all(len(t) > 3 for t in ref["tokens_alone"])


@pytest.mark.skipif(not C.have_reference(), reason="no checkout of the reference here")
def test_fixtures_equal_a_fresh_run():
    import subprocess
    import sys

    out = subprocess.run([sys.executable, "tools/gen_rnnt_fixtures.py", "--check"], cwd=C.ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-800:]
