"""Detail sessions, model.stream_detailed(...) (streaming.StreamingRecognizer: the detail variants of the mode-2 search for a transducer,
tfasr_ctc_greedy_decode_carry_detail on a carried state for a CTC head), for each of the seven streamable classes on the tiny f32 configs
and utterances of the existing stream tests; three streams of unequal length.

After finish(), stream b's record (rec.recognized()) is what model.recognize_detailed gives utterance b ALONE: tokens, frames and ends
exactly; log-probabilities, entropies and scores at the whole-step bar of DESIGN.md 4b-2 (rtol 1e-3, atol 1e-4: the session's encoder
frames are the offline ones only up to that bar for the attention models).  That holds for one accept of everything and for many small
uneven accepts.  The per-call outputs' first three fields are those of a plain model.stream(...) session fed the same calls, every token a call
reports closed holds the bits the final record holds, nothing is open after finish(), and trailing_blank_frames() is the record's."""
import numpy as np
import pytest
import torch

from tensorflowasr_amd import schemas
from tensorflowasr_amd.schemas import PredictInput
from tensorflowasr_amd.streaming import StreamDetailOutput, StreamOutput

import stream_oracle as SO

pytestmark = pytest.mark.gpu
BAR = dict(rtol=1e-3, atol=1e-4)
PATTERNS = {"whole": None, "uneven": [733, 160, 4001, 57]}
_CASES = {}


# =============================================================================================== the seven models
def _conformer(dev, head, dtype=torch.float32):
    from test_stream_gpu import _tiny

    if head == "ctc":
        return dict(model=_tiny(dev, dtype, head="ctc"), sigs=SO.noise(5, [1.7, 3.0, 2.2]), kw={})
    z, _ = SO.load_golden()
    model = _tiny(dev, dtype, {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("W/")})
    model.ps.p("joint/vocab/b")[0] += 0.5  # (tests/test_stream_gpu.py: the input condition under which the session equals recognize)
    return dict(model=model, sigs=SO.noise(1, [1.7, 3.0, 2.2]), kw=dict(precision="f32" if dtype == torch.float32 else "bf16"))


def _transformer(dev, head):
    import transformer_cases as TC
    from tensorflowasr_amd.transformer import TransformerCTC, TransformerTransducer
    from test_transformer_stream_gpu import build

    model = build(dev) if head == "ctc" else build(dev, cls=TransformerTransducer, head="rnnt")
    assert isinstance(model, TransformerCTC if head == "ctc" else TransformerTransducer)
    sig = TC.audio()
    return dict(model=model, sigs=[np.ascontiguousarray(sig[b, :n]) for b, n in enumerate(TC.SAMPLES)], kw={})


def _conv_ctc(dev, which):
    if which == "jasper":
        from test_jasper_gpu import build

        model, seed = build(dev, torch.float32), 21
    else:
        from test_ds2_gpu import build

        model, seed = build(dev, "uni", torch.float32), 5
    model.decode_precision = "f32"
    rng = np.random.default_rng(seed)
    sigs = [np.clip(rng.standard_normal(n) * 0.1, -1, 1).astype(np.float32) for n in (4960, 7361, 12800)]
    return dict(model=model, sigs=sigs, kw=dict(chunk_frames=8, precision="f32"))


def _rnnt(dev):
    import rnnt_cases as RC
    from test_rnnt_model_gpu import build

    model = build(dev, "ln", torch.float32)
    model.decode_precision = "f32"
    a = RC.audio()
    return dict(model=model, sigs=[a[b, :n].copy() for b, n in enumerate(RC.SAMPLES)], kw=dict(chunk_frames=8, precision="f32"))


BUILD = {
    "ConformerTransducer": lambda dev: _conformer(dev, "transducer"), "ConformerCTC": lambda dev: _conformer(dev, "ctc"),
    "TransformerCTC": lambda dev: _transformer(dev, "ctc"), "TransformerTransducer": lambda dev: _transformer(dev, "rnnt"),
    "JasperCTC": lambda dev: _conv_ctc(dev, "jasper"), "DeepSpeech2CTC": lambda dev: _conv_ctc(dev, "ds2"), "RnnTransducer": _rnnt,
}


def case(dev, name):
    """the model, its three utterances and recognize_detailed of each ALONE: built once per class, shared by the arrival patterns"""
    if name not in _CASES:
        c = BUILD[name](dev)
        assert type(c["model"]).__name__ == name
        c["alone"] = [_alone(c["model"], s) for s in c["sigs"]]
        _CASES[name] = c
    return _CASES[name]


def _alone(model, sig):
    x = PredictInput(torch.from_numpy(sig[None].copy()), torch.tensor([len(sig)], dtype=torch.int32))
    det = model.recognize_detailed(x)
    there = (det.frames[0] >= 0).cpu()
    pick = lambda t: t[0].cpu()[there]
    return dict(tokens=pick(det.predict.tokens).tolist(), frames=pick(det.frames).tolist(), ends=None if det.ends is None else pick(det.ends).tolist(),
                logp=pick(det.log_probs).numpy(), ent=pick(det.entropies).numpy(), score=float(det.scores[0]))


# =============================================================================================== feeding
def calls_of(sigs, pieces):
    """the accept calls of an arrival pattern: [(pcm [B, n], lengths)]; None = everything in one call"""
    B, n = len(sigs), max(len(s) for s in sigs)
    pieces = pieces or [n]
    calls, p0, k = [], 0, 0
    while p0 < n:
        piece = pieces[k % len(pieces)]
        x = np.zeros((B, piece), np.float32)
        lens = []
        for b, s in enumerate(sigs):
            seg = s[p0:p0 + piece]
            x[b, :len(seg)] = seg
            lens.append(len(seg))
        calls.append((torch.from_numpy(x), lens))
        p0, k = p0 + piece, k + 1
    return calls


def run(rec, calls, between=None):
    outs = []
    for x, lens in calls:
        outs.append(rec.accept(x, lens))
        if between is not None:
            between(rec, outs[-1])
    outs.append(rec.finish())
    return outs


def record_rows(out):
    """RecognizeOutput -> per row dict of the columns that hold a token"""
    rows = []
    for b in range(out.frames.shape[0]):
        there = out.frames[b] >= 0
        assert there.int().sum() == 0 or bool(there[:int(there.sum())].all())  # the tokens fill the row from column 0
        rows.append(dict(tokens=out.predict.tokens[b][there].tolist(), frames=out.frames[b][there].tolist(),
                         ends=None if out.ends is None else out.ends[b][there].tolist(), logp=out.log_probs[b][there].numpy(),
                         ent=out.entropies[b][there].numpy(), score=float(out.scores[b])))
    return rows


def midway(rec, out):
    """after every accept: the record is consistent with the flags, and an open token ends at the frames seen so far"""
    rows, op, trail = record_rows(rec.recognized()), rec.open_tokens().tolist(), rec.trailing_blank_frames().tolist()
    for b, r in enumerate(rows):
        seen = int(out.frames[b])
        if op[b]:
            assert rec.ctc and r["ends"][-1] == seen and trail[b] == 0
        else:
            last_end = 0 if not r["tokens"] else (r["ends"][-1] if rec.ctc else r["frames"][-1] + 1)
            assert trail[b] == seen - last_end


# =============================================================================================== the tests
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("name", list(BUILD))
def test_the_record_is_recognize_detailed_alone(dev, name, pattern):
    c = case(dev, name)
    model, sigs, B = c["model"], c["sigs"], len(c["sigs"])
    calls = calls_of(sigs, PATTERNS[pattern])
    rec = model.stream_detailed(B, **c["kw"])
    outs = run(rec, calls, midway)
    plain = run(model.stream(B, **c["kw"]), calls)
    final = record_rows(rec.recognized())
    assert sum(len(r["tokens"]) for r in final) > 0
    assert not rec.open_tokens().any()
    # 1. each stream's record against recognize_detailed of its utterance alone
    for b, (got, want) in enumerate(zip(final, c["alone"])):
        assert got["tokens"] == want["tokens"] and got["frames"] == want["frames"] and got["ends"] == want["ends"], (b, got, want)
        np.testing.assert_allclose(got["logp"], want["logp"], **BAR)
        np.testing.assert_allclose(got["ent"], want["ent"], **BAR)
        np.testing.assert_allclose(got["score"], want["score"], **BAR)
    assert (rec.recognized().ends is None) == (not rec.ctc)
    # 2. the first three fields are the plain session's, call by call
    for d, p in zip(outs, plain):
        assert isinstance(d, StreamDetailOutput) and type(p) is StreamOutput and p._fields == ("tokens", "tokens_length", "frames")
        assert torch.equal(d.tokens, p.tokens) and torch.equal(d.tokens_length, p.tokens_length) and torch.equal(d.frames, p.frames)
        assert d.token_frames.shape == d.tokens.shape == d.log_probs.shape == d.entropies.shape
        assert (d.token_ends is None) == (not rec.ctc)
    # 3. every token a call reports closed holds the bits the final record holds
    at, closed = [0] * B, 0
    for d in outs:
        for b in range(B):
            for i in range(int(d.tokens_length[b])):
                k, r = at[b] + i, final[b]
                assert int(d.tokens[b, i]) == r["tokens"][k] and int(d.token_frames[b, i]) == r["frames"][k]
                if rec.ctc and int(d.token_ends[b, i]) < 0:
                    assert i == int(d.tokens_length[b]) - 1  # only a call's last token can be open
                    continue
                closed += 1
                assert not rec.ctc or int(d.token_ends[b, i]) == r["ends"][k]
                assert float(d.log_probs[b, i]) == float(r["logp"][k]) and float(d.entropies[b, i]) == float(r["ent"][k])
            pad = slice(int(d.tokens_length[b]), None)
            assert (d.token_frames[b, pad] == -1).all() and (d.log_probs[b, pad] == 0).all() and (d.entropies[b, pad] == 0).all()
            at[b] += int(d.tokens_length[b])
    assert at == [len(r["tokens"]) for r in final] and closed > 0
    # 4. the frames since the last token
    frames = outs[-1].frames.tolist()
    want = [frames[b] - (0 if not r["tokens"] else (r["ends"][-1] if rec.ctc else r["frames"][-1] + 1)) for b, r in enumerate(final)]
    assert rec.trailing_blank_frames().tolist() == want
    # 5. rows= picks streams; a reset stream starts an empty record
    one = record_rows(rec.recognized(rows=[2]))
    assert len(one) == 1 and one[0]["tokens"] == final[2]["tokens"]
    rec.reset(rows=[1])
    after = record_rows(rec.recognized())
    assert after[1]["tokens"] == [] and after[0]["tokens"] == final[0]["tokens"] and rec.trailing_blank_frames().tolist()[1] == 0


def test_word_details_reads_the_record(dev):
    c = case(dev, "TransformerCTC")
    model, sigs = c["model"], c["sigs"]
    rec = model.stream_detailed(3)
    run(rec, calls_of(sigs, [4000]))
    out = rec.recognized()
    times, conf = schemas.token_times(out), schemas.token_confidences(out)
    assert times.shape == out.frames.shape and ((conf >= 0) & (conf <= 1)).all()
    words = 0
    for b in range(3):
        rows = schemas.word_details(out, model.tokenizer, b)
        end_of_stream = rec.frames[b] * out.seconds_per_frame
        for word, start, end, logp, confidence in rows:
            assert isinstance(word, str) and word and 0 <= start < end <= end_of_stream + 1e-9 and logp <= 0 and 0 <= confidence <= 1
        assert [r[1] for r in rows] == sorted(r[1] for r in rows)
        words += len(rows)
    assert words > 0


def test_a_bf16_conformer_session_is_well_formed(dev):
    c = _conformer(dev, "transducer", torch.bfloat16)
    rec = c["model"].stream_detailed(3, **c["kw"])
    outs = run(rec, calls_of(c["sigs"], [4000]))
    out = rec.recognized()
    assert out.ends is None and not rec.open_tokens().any()
    for b, r in enumerate(record_rows(out)):
        assert r["frames"] == sorted(r["frames"]) and all(0 <= f < rec.frames[b] for f in r["frames"])
        assert (r["logp"] <= 0).all() and (r["ent"] >= 0).all() and np.isfinite(r["logp"]).all() and np.isfinite(r["ent"]).all()
    assert sum(int(o.tokens_length.sum()) for o in outs) == sum(len(r["tokens"]) for r in record_rows(out))


def test_a_plain_session_has_no_record(dev):
    rec = case(dev, "JasperCTC")["model"].stream(1, chunk_frames=8)
    for call in (rec.recognized, rec.open_tokens, rec.trailing_blank_frames):
        with pytest.raises(ValueError, match="stream_detailed"):
            call()
