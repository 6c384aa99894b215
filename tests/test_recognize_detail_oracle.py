"""CPU: pin tests/recognize_detail_oracle.py (what the GPU tests of recognize_detailed compare against) to tests/decode_oracle.py and to
first principles, in float32, and pin schemas.token_confidences / word_details on a hand-written RecognizeOutput."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import conformer_ref as R
from tensorflowasr_amd import schemas
from tensorflowasr_amd import tokenizers as tk

import decode_oracle as DO
import recognize_detail_oracle as RD

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "librispeech")
B, T = 5, 9
LENS = [9, 4, 7, 1, 6]


def _case(seed=12, blank_bias=0.0, sharpen=4.0):
    """the weights and inputs of tests/test_decode_oracle.py"""
    W = R.init_weights(R.conformer_config("tiny"), seed=seed, scale_bias=0.1)
    W["joint/vocab/w"] = W["joint/vocab/w"] * sharpen
    W["joint/vocab/b"] = W["joint/vocab/b"].clone()
    W["joint/vocab/b"][0] += blank_bias
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(B, T, W["joint/enc/w"].shape[0], generator=g) * 2
    encj = torch.cat([enc[:, t:t + 1] @ W["joint/enc/w"] + W["joint/enc/b"] for t in range(T)], 1)
    return W, encj


def _replay(mode, W, encj, lens):
    """the float32 search once more, by hand: per written column, (frame_of before the update, log_softmax of the step's logits at the token)"""
    encj = encj.float()
    Bn, Tn, _ = encj.shape
    P = W["pred/lstm/rk"].shape[0]
    max_tokens = int(lens[0]) * 3 if mode == 1 else 2 * Tn + 1
    st = DO.new_state(mode, Bn, P, lens, max_tokens)
    seen = {}
    for _ in range(Tn + max_tokens + 2):  # (decode_oracle.search's cap: a saturated row keeps the condition true for ever)
        if not DO.active(mode, st["nframes"], st["frame_idx"], st["tok_idx"], max_tokens):
            break
        c_new, h_new, _, logits = DO.step(W, st["prev_tok"], st["h"], st["c"], encj, st["nframes"], st["frame_idx"], Tn, True, torch.float32)
        frame = DO.frame_of(st["nframes"], st["frame_idx"], Tn).numpy()
        lsm = torch.log_softmax(logits, -1)
        H = -(torch.exp(lsm) * lsm).sum(-1)
        new = DO.update(mode, logits, st, h_new.numpy(), c_new.numpy(), max_tokens)
        cur = lsm.argmax(-1)
        for b in range(Bn):
            emitted = int(cur[b]) != 0 and (mode == 1 or (st["tok_idx"][b] < max_tokens and st["frame_idx"][b] <= st["nframes"][b]))
            if emitted:
                seen[(b, int(new["tok_idx"][b]))] = (int(frame[b]), float(lsm[b, cur[b]]), float(H[b]), int(cur[b]))
        st = new
    return st, seen


@pytest.mark.parametrize("mode", [0, 1])
def test_recorder_follows_the_search_and_records_the_decision(mode):
    n_tokens = 0
    for bias in (0.0, 2.0, 4.0):
        W, encj = _case(blank_bias=bias)
        rows = [(encj, LENS)] if mode == 0 else [(encj[b:b + 1, :n], [n]) for b, n in enumerate(LENS)]
        for e, lens in rows:
            ref = DO.search(mode, W, e, lens, dtype=torch.float32)
            st, det = RD.search(mode, W, e, lens, dtype=torch.float32)
            for k in ("tokens", "prev_tok", "tok_idx", "frame_idx", "h", "c"):
                np.testing.assert_array_equal(st[k], ref[k], err_msg=k)
            _, seen = _replay(mode, W, e, lens)
            present = det["frames"] >= 0
            assert set(zip(*np.nonzero(present))) == set(seen)  # details exactly at the columns a symbol was written to
            for (b, col), (frame, lp, H, cur) in seen.items():
                assert st["tokens"][b, col] == cur
                assert det["frames"][b, col] == frame and frame < lens[b]
                assert np.float32(det["logp"][b, col]) == np.float32(lp)
                np.testing.assert_allclose(det["entropy"][b, col], H, rtol=1e-6)
            assert (det["logp"][~present] == 0).all() and (det["entropy"][~present] == 0).all()
            assert (det["logp"][present] < 0).all() and (det["entropy"][present] > 0).all()
            if mode == 0:
                assert not present[:, :2].any()  # recognize_batch's layout: symbols from column 2
                for b in range(len(lens)):
                    f = det["frames"][b][present[b]]
                    assert (np.diff(f) >= 0).all()
            else:
                f = det["frames"][0][present[0]]
                assert (np.diff(f) >= 0).all() and (np.bincount(f, minlength=1) <= 3).all()
            n_tokens += int(present.sum())
    assert n_tokens > 20


def test_entropy_ignores_classes_of_probability_zero():
    lsm = torch.log_softmax(torch.tensor([[0.0, -math.inf, 0.0, -1e4]], dtype=torch.float64), -1)
    H = RD.entropy(lsm)
    assert torch.isfinite(H).all() and H[0].item() == pytest.approx(math.log(2.0), rel=1e-12)
    assert RD.entropy(torch.log_softmax(torch.zeros(1, 8, dtype=torch.float64), -1))[0].item() == pytest.approx(math.log(8.0), rel=1e-12)


def test_update_detail_leaves_the_buffers_alone_where_no_symbol_is_written():
    """mode 2: a finished row, a blank and a symbol dropped past the buffer write nothing; a symbol writes its column"""
    V, P, max_tokens = 12, 4, 6
    cur, fi, nf, pf, ti = [9, 0, 5, 7], [4, 1, 1, 1], [4, 4, 4, 4], [1, 2, 0, 0], [2, 2, 2, 5]
    logits = torch.zeros(4, V)
    logits[torch.arange(4), torch.tensor(cur)] = 9.0
    st = dict(nframes=np.array(nf), frame_idx=np.array(fi), prev_tok=np.full(4, 3), tok_idx=np.array(ti), tokens=np.full((4, max_tokens), 33),
              per_frame=np.array(pf), h=np.zeros((4, P), np.float32), c=np.zeros((4, P), np.float32))
    det = RD.new_detail(st["tokens"])
    new, det2, written = RD.update_detail(2, logits, st, det, np.ones((4, P), np.float32), np.ones((4, P), np.float32), max_tokens, T=6)
    assert written.tolist() == [False, False, True, False]
    assert (det2["frames"] >= 0).sum() == 1 and det2["frames"][2, 3] == 1 and new["tokens"][2, 3] == 5
    assert det2["logp"][2, 3] == pytest.approx(float(torch.log_softmax(logits[2].double(), -1)[5]), rel=1e-12)


def test_ctc_oracle_is_the_collapse_of_the_frame_argmax():
    g = torch.Generator().manual_seed(3)
    Bc, Tc, V = 6, 40, 5
    x = (torch.randn(Bc, Tc, V, generator=g) * 2).numpy().astype(np.float32)
    x[:, :, 0] += 1.0
    x[0, 5:9] = x[0, 5]  # a run of equal frames
    lens = [40, 0, 1, 17, 40, 33]
    out = RD.ctc_greedy_detail(x, lens, blank=0, dtype=np.float32)
    lsm = torch.log_softmax(torch.from_numpy(x), -1).numpy()
    n_tok = 0
    for b in range(Bc):
        am = x[b, :lens[b]].argmax(-1)
        want = [int(c) for t, c in enumerate(am) if c != 0 and (t == 0 or am[t - 1] != c)]
        n = int(out["tokens_len"][b])
        assert out["tokens"][b, :n].tolist() == want and (out["tokens"][b, n:] == 0).all()
        assert (out["starts"][b, n:] == -1).all() and (out["ends"][b, n:] == -1).all() and (out["logp"][b, n:] == 0).all()
        np.testing.assert_allclose(out["score"][b], lsm[b, :lens[b]].max(-1).sum(), rtol=1e-5, atol=1e-6)
        prev_end = 0
        for i in range(n):
            s, e = int(out["starts"][b, i]), int(out["ends"][b, i])
            assert prev_end <= s < e <= lens[b] and (am[s:e] == want[i]).all()
            assert s == 0 or am[s - 1] != want[i]
            assert e == lens[b] or am[e] != want[i]
            np.testing.assert_allclose(out["logp"][b, i], lsm[b, s:e, want[i]].sum(), rtol=1e-5, atol=1e-6)
            assert 0 < out["entropy"][b, i] <= math.log(V) + 1e-6
            prev_end = e
        n_tok += n
    assert out["tokens_len"][1] == 0 and out["score"][1] == 0 and n_tok > 30
    # the tokens and the score are at least as probable as any labelling's best path: the score bounds every token sum
    assert (out["logp"].sum(1) >= out["score"] - 1e-4).all()


def _hand_ctc():
    predict = schemas.PredictOutput(tokens=torch.tensor([[0, 0, 0, 0, 0]], dtype=torch.int32), next_tokens=None)
    return schemas.RecognizeOutput(predict, frames=torch.tensor([[2, 4, 7, 9, -1]], dtype=torch.int32),
                                   ends=torch.tensor([[4, 5, 9, 10, -1]], dtype=torch.int32),
                                   log_probs=torch.tensor([[2 * math.log(0.5), math.log(0.9), 2 * math.log(0.8), math.log(0.25), 0.0]]),
                                   entropies=torch.tensor([[math.log(29.0), 0.0, 0.5 * math.log(29.0), 0.1, 0.0]]),
                                   scores=torch.tensor([-3.0]), seconds_per_frame=0.04, vocab_size=29)


def test_token_confidences_and_times():
    out = _hand_ctc()
    np.testing.assert_allclose(schemas.token_confidences(out).numpy(), [[0.5, 0.9, 0.8, 0.25, 0.0]], rtol=1e-6)
    np.testing.assert_allclose(schemas.token_confidences(out, "prob").numpy(), [[0.5, 0.9, 0.8, 0.25, 0.0]], rtol=1e-6)
    np.testing.assert_allclose(schemas.token_confidences(out, "entropy").numpy(), [[0.0, 1.0, 0.5, 1 - 0.1 / math.log(29.0), 0.0]], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(schemas.token_times(out).numpy(), [[0.08, 0.16, 0.28, 0.36, -1.0]], rtol=1e-6)
    rnnt = out._replace(ends=None)  # a transducer: one decision per token
    np.testing.assert_allclose(schemas.token_confidences(rnnt).numpy(), [[0.25, 0.9, 0.64, 0.25, 0.0]], rtol=1e-6)
    with pytest.raises(ValueError):
        schemas.token_confidences(out, "margin")
    assert schemas.RecognizeOutput._fields == ("predict", "frames", "ends", "log_probs", "entropies", "scores", "seconds_per_frame", "vocab_size")


def test_word_details_with_the_char_tokenizer():
    t = tk.get({"type": "characters", "blank_index": 0, "vocabulary": f"{REF}/characters/english.vocab"})
    ids = t.tokenize("ab cd")  # a b ' ' c d
    out = _hand_ctc()
    out = out._replace(predict=out.predict._replace(tokens=torch.as_tensor(np.asarray(ids)).to(torch.int32)[None]),
                       frames=torch.tensor([[2, 4, 6, 7, 9]], dtype=torch.int32), ends=torch.tensor([[4, 5, 7, 9, 10]], dtype=torch.int32),
                       log_probs=torch.tensor([[2 * math.log(0.5), math.log(0.9), math.log(0.7), 2 * math.log(0.8), math.log(0.25)]]),
                       entropies=torch.zeros(1, 5))
    words = schemas.word_details(out, t, 0)
    assert [w[0] for w in words] == ["ab", "cd"]
    assert words[0][1:3] == (pytest.approx(0.08), pytest.approx(0.20)) and words[1][1:3] == (pytest.approx(0.28), pytest.approx(0.40))
    assert words[0][3] == pytest.approx(2 * math.log(0.5) + math.log(0.9)) and words[0][4] == pytest.approx(0.5)
    assert words[1][3] == pytest.approx(2 * math.log(0.8) + math.log(0.25)) and words[1][4] == pytest.approx(0.25)
    # a transducer batch row: blanks in columns 0, 1 and behind the symbols; a word ends one frame after its last token's frame
    row = np.concatenate([[0, 0], ids, [0, 0]]).astype(np.int32)
    fr = torch.tensor([[-1, -1, 1, 1, 2, 3, 5, -1, -1]], dtype=torch.int32)
    lp = torch.where(fr >= 0, torch.full((1, 9), math.log(0.5)), torch.zeros(1, 9))
    lp[0, 5] = math.log(0.125)
    rn = schemas.RecognizeOutput(schemas.PredictOutput(torch.from_numpy(row)[None], None), fr, None, lp, torch.zeros(1, 9), lp.sum(1), 0.04, 29)
    words = schemas.word_details(rn, t, 0)
    assert [(w[0], w[1], w[2]) for w in words] == [("ab", pytest.approx(0.04), pytest.approx(0.08)), ("cd", pytest.approx(0.12), pytest.approx(0.24))]
    assert words[1][3] == pytest.approx(math.log(0.125) + math.log(0.5)) and words[1][4] == pytest.approx(0.125)


def test_word_details_with_the_sentencepiece_tokenizer():
    pytest.importorskip("sentencepiece")
    path = f"{REF}/sentencepiece/train_bpe_1000.model"
    if not os.path.exists(path):
        pytest.skip("no BPE model on this machine")
    t = tk.get({"type": "sentencepiece", "blank_index": 0, "vocabulary": path})
    ids = np.asarray(t.tokenize("stew for dinner"))
    n = len(ids)
    spans = t.word_spans(ids)
    assert [w for w, _, _ in spans] == ["stew", "for", "dinner"]
    starts = torch.arange(n, dtype=torch.int32)[None] * 3
    conf = 0.3 + 0.6 * torch.rand(1, n, generator=torch.Generator().manual_seed(1))
    out = schemas.RecognizeOutput(schemas.PredictOutput(torch.from_numpy(ids.astype(np.int32))[None], None), starts, starts + 2, 2 * torch.log(conf),
                                  torch.zeros(1, n), torch.tensor([0.0]), 0.04, 1000)
    words = schemas.word_details(out, t, 0)
    assert len(words) == 3
    for (word, s, e, lp, c), (w, a, b) in zip(words, spans):
        assert word == w and s == pytest.approx(0.04 * 3 * a) and e == pytest.approx(0.04 * (3 * b + 2))
        assert lp == pytest.approx(float(2 * torch.log(conf[0, a:b + 1]).sum()), rel=1e-5) and c == pytest.approx(float(conf[0, a:b + 1].min()), rel=1e-5)
