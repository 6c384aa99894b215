"""tfasr_ctc_beam_search: the device prefix beam search decodes exactly like the host routine tfasr_ctc_beam_search_host (and the
oracle's textbook search), keeps one trie node per label sequence, keeps the exact-tie order, returns an exact n-best list when
the beam holds every prefix, accepts bf16 logits, and is deterministic at the bench shape."""
import itertools

import numpy as np
import pytest
import torch

from oracle import ctc_ref
from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

pytestmark = pytest.mark.gpu


def host(x, lens, beam, blank):
    """tfasr_ctc_beam_search_host on a numpy [B,T,V] batch -> tokens [B,T], lengths [B], log_prob [B]"""
    x = np.ascontiguousarray(x, np.float32)
    B, T, V = x.shape
    ln = np.asarray(lens, np.int32)
    toks, n, lp = np.zeros((B, T), np.int32), np.zeros(B, np.int32), np.zeros(B, np.float32)
    st = _lib.load().tfasr_ctc_beam_search_host(x.ctypes.data, ln.ctypes.data, B, T, V, beam, blank, toks.ctypes.data, n.ctypes.data,
                                                lp.ctypes.data)
    assert st == 0
    return toks, n, lp


def device(x, lens, beam, blank, top_paths=1, dtype=torch.float32):
    xt = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to("cuda", dtype)
    torch.cuda.synchronize()
    out = K.ctc_beam_search_device(xt, torch.tensor(lens, dtype=torch.int32), beam_width=beam, top_paths=top_paths, blank_index=blank)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def assert_same_as_host(x, lens, beam, blank, lp_tol=1e-4, what=""):
    ht, hn, hlp = host(x, lens, beam, blank)
    dt, dn, dlp = device(x, lens, beam, blank)
    np.testing.assert_array_equal(dn[:, 0], hn, err_msg=what)
    np.testing.assert_array_equal(dt[:, 0], ht, err_msg=what)
    np.testing.assert_allclose(dlp[:, 0], hlp, rtol=0, atol=lp_tol, err_msg=what)
    return dt, dn, dlp


@pytest.mark.parametrize("V", [5, 29, 1000])
def test_parity_with_host_routine_and_oracle(dev, V):
    rng = np.random.default_rng(V)
    B, T = 8, 60
    lens = [60, 0, 1, 37, 60, 12, 59, 2]
    for beam in (1, 2, 4, 10, 16, 64):
        for blank in (0, V - 1):
            scale = (2.0, 3.0, 4.0)[beam % 3]
            x = (rng.standard_normal((B, T, V)) * scale).astype(np.float32)
            dt, dn, _ = assert_same_as_host(x, lens, beam, blank, what=f"V={V} beam={beam} blank={blank}")
            if V <= 29 and beam <= 10:
                for b, Tb in enumerate(lens):
                    lab, _ = ctc_ref.ctc_beam_search(x[b], Tb, beam, blank)
                    assert dt[b, 0, :dn[b, 0]].tolist() == lab, (V, beam, blank, b)


def test_prefix_reentry_small_alphabet_narrow_beam(dev):
    """a prefix that leaves the beam and comes back while one of its extensions stayed keeps ONE node (its mass merges)"""
    rng = np.random.default_rng(5)
    for beam in (2, 3):
        x = (rng.standard_normal((300, 14, 3)) * 1.5).astype(np.float32)
        assert_same_as_host(x, [14] * 300, beam, 0, what=f"beam={beam}")
        dt, dn, _ = device(x, [14] * 300, beam, 0)
        for b in range(0, 300, 15):
            lab, _ = ctc_ref.ctc_beam_search(x[b], 14, beam, 0)
            assert dt[b, 0, :dn[b, 0]].tolist() == lab


def test_exact_ties_follow_label_sequence_order(dev):
    rng = np.random.default_rng(11)
    # duplicated columns: classes 1 and 3 (and 2 and 4) always score the same
    base = (rng.standard_normal((6, 20, 3)) * 2.0).astype(np.float32)
    dup = np.concatenate([base, base[:, :, 1:3], np.full((6, 20, 1), -1.0, np.float32)], axis=2)  # V = 6, blank 5 or 0
    for beam in (1, 2, 4, 10):
        assert_same_as_host(dup, [20, 19, 7, 1, 20, 3], beam, 5, what=f"dup beam={beam}")
        assert_same_as_host(dup, [20, 19, 7, 1, 20, 3], beam, 0, what=f"dup blank0 beam={beam}")
    # all-equal rows: every candidate of a frame ties with its siblings
    flat = np.zeros((4, 9, 4), np.float32)
    flat[1] = 0.5
    flat[2, :, :] = rng.standard_normal((9, 1)).astype(np.float32)
    for beam in (1, 3, 8, 16):
        for blank in (0, 3):
            assert_same_as_host(flat, [9, 8, 5, 2], beam, blank, what=f"flat beam={beam} blank={blank}")


def _enumerate_labellings(x, blank):
    """every labelling's total probability by summing all alignments (f64)"""
    lp = x.astype(np.float64) - np.logaddexp.reduce(x.astype(np.float64), axis=1, keepdims=True)
    T, V = lp.shape
    tot = {}
    for path in itertools.product(range(V), repeat=T):
        lab, prev = [], None
        for c in path:
            if c != blank and c != prev:
                lab.append(c)
            prev = c
        k = tuple(lab)
        tot[k] = np.logaddexp(tot.get(k, -np.inf), sum(lp[t, c] for t, c in enumerate(path)))
    return sorted(tot.items(), key=lambda kv: (-kv[1], kv[0]))


def test_nbest_exact_with_a_wide_beam(dev):
    rng = np.random.default_rng(3)
    B, T, V, P = 6, 5, 3, 8
    lens = [5, 4, 5, 4, 5, 1]
    for blank in (0, 2):
        x = (rng.standard_normal((B, T, V)) * 2.0).astype(np.float32)
        toks, n, lp = device(x, lens, 64, blank, top_paths=P)
        for b, Tb in enumerate(lens):
            want = _enumerate_labellings(x[b, :Tb], blank)
            for p in range(P):
                if p < len(want):
                    lab, wlp = want[p]
                    assert toks[b, p, :n[b, p]].tolist() == list(lab), (blank, b, p)
                    assert not toks[b, p, n[b, p]:].any()
                    assert abs(lp[b, p] - wlp) < 1e-5, (blank, b, p, lp[b, p], wlp)
                else:  # fewer labellings than paths: empty, length 0
                    assert n[b, p] == 0 and not toks[b, p].any() and lp[b, p] == -np.inf
        # the top path equals the host routine's
        ht, hn, _ = host(x, lens, 64, blank)
        np.testing.assert_array_equal(toks[:, 0], ht)
        np.testing.assert_array_equal(n[:, 0], hn)


def test_bf16_logits_decode_like_their_f32_upcast(dev):
    rng = np.random.default_rng(8)
    x = torch.from_numpy((rng.standard_normal((8, 40, 29)) * 3.0).astype(np.float32)).to(torch.bfloat16)
    x32 = x.float().numpy()
    lens = [40, 33, 1, 0, 40, 17, 28, 39]
    for beam in (1, 4, 10):
        a = device(x32, lens, beam, 28, top_paths=min(beam, 3), dtype=torch.bfloat16)
        b = device(x32, lens, beam, 28, top_paths=min(beam, 3), dtype=torch.float32)
        for u, v in zip(a, b):
            np.testing.assert_array_equal(u, v)


def test_model_device_search_matches_host_and_oracle(dev):
    from oracle import conformer_ref as R
    from tensorflowasr_amd import configs
    from tensorflowasr_amd.ctc_model import ConformerCTC
    from tensorflowasr_amd.schemas import PredictInput, TrainData, TrainInput, TrainLabel

    cfg = configs.conformer_tiny(head="ctc", mhsam_use_attention_bias=True)
    ocfg = R.conformer_config("tiny")
    ocfg.update(head="ctc", mhsam_use_attention_bias=True)
    model = ConformerCTC(cfg, dev, dtype=torch.float32, seed=2)
    model.ps.import_keras(R.init_weights(ocfg, seed=3, scale_bias=0.1))
    rng = np.random.default_rng(2)
    lens, ulens, U = [4000, 4000, 2500], [3, 2, 2], 4
    B = len(lens)
    sig = np.clip(rng.standard_normal((B, 4000)) * 0.1, -1, 1).astype(np.float32)
    for b, n in enumerate(lens):
        sig[b, n:] = 0.0
    labels = rng.integers(1, cfg.vocab_size, (B, U)).astype(np.int32)
    for b, u in enumerate(ulens):
        labels[b, u:] = 0
    data = TrainData(TrainInput(torch.from_numpy(sig), torch.tensor(lens, dtype=torch.int32), torch.zeros(B, 1, dtype=torch.int32),
                                torch.ones(B, dtype=torch.int32)),
                     TrainLabel(torch.from_numpy(labels), torch.tensor(ulens, dtype=torch.int32)))
    model.optimizer["schedule"] = 3e-3
    for _ in range(20):  # a few steps, so that the decisions are not near-ties
        model.train_step(data, masks=(None, None))
    inp = PredictInput(torch.from_numpy(sig), torch.tensor(lens, dtype=torch.int32))
    for beam in (1, 4, 10):
        host_out = model.recognize_beam(inp, beam_width=beam).tokens.cpu().numpy()
        dev_out = model.recognize_beam(inp, beam_width=beam, device_search=True).tokens.cpu().numpy()
        np.testing.assert_array_equal(dev_out, host_out)
        logits, elen = model._infer_logits(inp)
        V = logits.shape[-1]
        for b in range(B):
            lab, _ = ctc_ref.ctc_beam_search(logits[b].float().cpu().numpy(), int(elen[b]), beam, blank=V - 1)
            assert list(dev_out[b][:len(lab)]) == lab and not dev_out[b][len(lab):].any()
        toks, n, lp = model.recognize_nbest(inp, beam_width=beam, top_paths=1)
        width = max(int(n.max()), 1)
        np.testing.assert_array_equal(toks[:, 0, :width].cpu().numpy(), dev_out)
    toks, n, lp = model.recognize_nbest(inp, beam_width=4, top_paths=4)
    lp = lp.cpu().numpy()
    assert toks.shape[:2] == (B, 4) and (np.diff(lp, axis=1) <= 0).all()


def test_deterministic_at_the_bench_shape(dev):
    from tensorflowasr_amd import configs
    from tensorflowasr_amd.ctc_model import ConformerCTC
    from tensorflowasr_amd.schemas import PredictInput

    cfg = configs.conformer_ctc_s()
    model = ConformerCTC(cfg, dev, dtype=torch.bfloat16, seed=0)
    rng = np.random.default_rng(0)
    B, n = 32, 160000
    sig = torch.from_numpy(np.clip(rng.standard_normal((B, n)).astype(np.float32) * 0.1, -1, 1)).to(dev)
    logits, elen = model._infer_logits(PredictInput(sig, torch.full((B,), n, dtype=torch.int32)))
    ln = torch.tensor(elen, dtype=torch.int32)
    torch.cuda.synchronize()
    a = K.ctc_beam_search_device(logits, ln, beam_width=10, top_paths=4)
    torch.cuda.synchronize()
    b = K.ctc_beam_search_device(logits, ln, beam_width=10, top_paths=4)
    torch.cuda.synchronize()
    assert a[0].shape == (B, 4, logits.shape[1])
    for u, v in zip(a, b):
        assert torch.equal(u.cpu(), v.cpu())
    assert (a[1][:, 0] >= 0).all() and torch.isfinite(a[2][:, 0]).all()
