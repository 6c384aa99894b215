"""model.evaluate end to end on tiny random-init models: the counts and rates it returns against host scoring of separate recognize /
recognize_beam / recognize_nbest calls, the results file, the beam column, the oracle row and the token error rate.

Four utterances of about a second, read from an ASRSliceDataset in batches of three, so the last batch holds one.  Tokenizers are the
LibriSpeech ones under tests/golden: characters for the Conformer transducer and the Conformer CTC model, the 256-piece SentencePiece
model for ContextNet.  The blank bias of each model is moved (BLANK_BIAS) so that its searches emit tokens: a test below refuses to pass
on empty hypotheses."""
import math
import os

import numpy as np
import pytest
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd import metrics as M
from tensorflowasr_amd import tokenizers as tk
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.contextnet import ContextNetTransducer
from tensorflowasr_amd.ctc_model import ConformerCTC
from tensorflowasr_amd.datasets import ASRSliceDataset, to_train_data
from tensorflowasr_amd.schemas import PredictInput

pytestmark = pytest.mark.gpu
REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "librispeech")
KINDS = ("conformer", "contextnet", "ctc")
# Added to the blank entry of the output bias (joint/vocab/b, or dec/logits/b for CTC); found on the device.  Greedy / beam tokens of the
# four utterances against 38 reference tokens (21 for ContextNet's pieces): Conformer 38 / 29 at +7 (at 0 the greedy search fills its token
# buffer, at +8 it says 10 tokens), CTC 63 / 61 at +6.  ContextNet's greedy search at this initialisation emits on every step (0 and below:
# the buffer fills, 222 tokens; its beam search 93) or never (+0.5 and above: 0 tokens), so its bias stays where it speaks.
BLANK_BIAS = {"conformer": 7.0, "contextnet": 0.0, "ctc": 6.0}
TEXTS = ["the cat sat", "he hoped", "stew for dinner", "it's"]
SAMPLES = [16000, 12800, 14400, 16000]
BATCH = 3


def build(kind, dev, blank_bias=None):
    if kind == "contextnet":
        tokenizer = tk.get({"type": "sentencepiece", "blank_index": 0, "vocabulary": f"{REF}/sentencepiece/train_bpe_256.model"})
        model = ContextNetTransducer(configs.contextnet_tiny(vocab_size=tokenizer.num_classes), dev, dtype=torch.float32, seed=3)
    else:
        tokenizer = tk.get({"type": "characters", "blank_index": 0, "vocabulary": f"{REF}/characters/english.vocab"})
        if kind == "ctc":
            model = ConformerCTC(configs.conformer_tiny(head="ctc", vocab_size=tokenizer.num_classes), dev, dtype=torch.float32, seed=3)
        else:
            model = ConformerTransducer(configs.conformer_tiny(vocab_size=tokenizer.num_classes), dev, dtype=torch.float32, seed=3)
    delta = BLANK_BIAS[kind] if blank_bias is None else blank_bias
    with torch.no_grad():
        if kind == "ctc":
            model.ps.p("dec/logits/w").mul_(3.0)
            model.ps.p("dec/logits/b")[model.blank] += delta
        else:  # a peaky joint and a token-sensitive prediction network, as the beam-search tests build them
            model.ps.p("joint/vocab/w").mul_(3.0)
            model.ps.p("pred/emb").mul_(3.0)
            model.ps.p("joint/vocab/b")[model.blank] += delta
    model.ps.refresh_shadow()
    model.tokenizer = tokenizer
    return model


def make_dataset(tokenizer, folder):
    rng = np.random.default_rng(11)
    audio = {f"utt{k}.wav": np.clip(rng.standard_normal(n) * 0.1, -1, 1).astype(np.float32) for k, n in enumerate(SAMPLES)}
    tsv = os.path.join(folder, "test.tsv")
    with open(tsv, "w", encoding="utf-8") as f:
        f.write("PATH\tDURATION\tTRANSCRIPT\n")
        for (name, x), text in zip(audio.items(), TEXTS):
            f.write(f"{name}\t{len(x) / 16000:.2f}\t{text}\n")
    # shuffle and drop_remainder are set on purpose: evaluate must read every entry, in file order, and leave the object alone
    return ASRSliceDataset("test", tokenizer, [tsv], shuffle=True, drop_remainder=True, reader=lambda path, sr: audio[os.path.basename(path)])


def batches(ds, dev):
    """the batches evaluate is specified to form: file order, BATCH at a time, the short last one included"""
    with open(ds.data_paths[0], encoding="utf-8") as f:
        entries = [ln.split("\t", 2) for ln in f.read().splitlines()[1:]]
    for s in range(0, len(entries), BATCH):
        yield to_train_data(ds.padded_batch([ds.parse(e[0], e[2]) for e in entries[s : s + BATCH]]), dev)


def predict_input(model, x):
    B = int(x.inputs.shape[0])
    return PredictInput(x.inputs, x.inputs_length, model.get_initial_tokens(batch_size=B), model.get_initial_encoder_states(batch_size=B),
                        model.get_initial_decoder_states(batch_size=B))


def compact(tokens, blank):
    """rows of search output -> (left-packed rows, lengths), by hand"""
    rows = [[int(v) for v in r if v >= 0 and v != blank] for r in np.asarray(tokens)]
    out = np.full((len(rows), max(max((len(r) for r in rows), default=0), 1)), -3, np.int32)
    for k, r in enumerate(rows):
        out[k, : len(r)] = r
    return out, np.asarray([len(r) for r in rows], np.int32)


def host_row(tokens_per_batch, label_batches, tokenizer, blank, cer_unit="char"):
    """ErrorStats (words, chars, tokens) and the texts of one results column, scored on the host from the searches' tokens"""
    stats = {u: M.ErrorStats() for u in ("words", "chars", "tokens")}
    texts, refs = [], []
    for toks, (labels, llen) in zip(tokens_per_batch, label_batches):
        h, hn = compact(toks, blank)
        stats["tokens"].update(M.edit_distance_host(h, labels, hn, llen))
        hyp_text = tokenizer.detokenize(np.asarray(toks))
        ref_text = tokenizer.detokenize(np.stack([np.where(np.arange(labels.shape[1]) < n, row, blank) for row, n in zip(labels, llen)]))
        stats["words"].update(M.edit_distance_host(*_reorder(M.encode_pairs(hyp_text, ref_text, "word"))))
        stats["chars"].update(M.edit_distance_host(*_reorder(M.encode_pairs(hyp_text, ref_text, cer_unit))))
        texts += hyp_text
        refs += ref_text
    return stats, texts, refs


def _reorder(enc):
    h, hn, r, rn = enc
    return h, r, hn, rn


def same_row(row, stats, utterances):
    assert row["words"] == stats["words"].counts() and row["chars"] == stats["chars"].counts() and row["tokens"] == stats["tokens"].counts()
    want = dict(M.summary(stats["words"], stats["chars"]), ter=stats["tokens"].error_rate)
    for k, v in want.items():
        assert row[k] == v or (math.isnan(row[k]) and math.isnan(v)), (k, row[k], v)
    assert row["utterances"] == utterances


@pytest.fixture(scope="module", params=KINDS)
def run(request, dev, tmp_path_factory):
    """everything computed once per model kind: the model, evaluate's three runs, and the separate searches with their host scores"""
    kind = request.param
    model = build(kind, dev)
    tok, blank = model.tokenizer, int(model.blank)
    folder = str(tmp_path_factory.mktemp(kind))
    ds = make_dataset(tok, folder)
    r = dict(kind=kind, model=model, ds=ds, tsv=os.path.join(folder, "results.tsv"))
    r["plain"] = model.evaluate(ds, output_file_path=r["tsv"], batch_size=BATCH)
    r["host_metrics"] = model.evaluate(ds, batch_size=BATCH, device_metrics=False)
    r["tsv_beam"] = os.path.join(folder, "results_beam.tsv")
    r["beam"] = model.evaluate(ds, output_file_path=r["tsv_beam"], names=["a", "b", "c", "d"], beam_width=4, top_paths=4, device_search=True,
                               batch_size=BATCH)
    r["beam_host_metrics"] = model.evaluate(list(batches(ds, dev)), beam_width=4, top_paths=4, device_search=True, device_metrics=False)
    greedy, beam, nbest, labels = [], [], [], []
    for x, y in batches(ds, dev):
        inp = predict_input(model, x)
        greedy.append(model.recognize(inp).tokens.cpu().numpy())
        beam.append(model.recognize_beam(inp, beam_width=4, device_search=True).tokens.cpu().numpy())
        nbest.append(tuple(t.cpu().numpy() for t in model.recognize_nbest(inp, beam_width=4, top_paths=4)))
        labels.append((y.labels.cpu().numpy().astype(np.int32), y.labels_length.cpu().numpy().astype(np.int32)))
    r.update(greedy=greedy, beam_tokens=beam, nbest=nbest, labels=labels, blank=blank)
    return r


def test_hypotheses_are_not_empty(run):
    said = sum(int(compact(t, run["blank"])[1].sum()) for t in run["greedy"])
    asked = sum(int(n.sum()) for _, n in run["labels"])
    print(f"{run['kind']}: greedy tokens {said}, beam tokens {sum(int(compact(t, run['blank'])[1].sum()) for t in run['beam_tokens'])}, "
          f"reference tokens {asked}")
    assert asked == sum(len(run["model"].tokenizer.tokenize(t)) for t in TEXTS) and asked > 0
    assert 2 * said >= asked


def test_counts_and_rates_equal_host_scoring_of_separate_searches(run):
    tok = run["model"].tokenizer
    stats, _, _ = host_row(run["greedy"], run["labels"], tok, run["blank"])
    same_row(run["plain"]["greedy"], stats, 4)
    same_row(run["plain"]["beam"], stats, 4)  # beam_width = 0: the beam column repeats the greedy one
    assert set(run["plain"]) == {"greedy", "beam"}
    same_row(run["beam"]["greedy"], stats, 4)
    stats, _, _ = host_row(run["beam_tokens"], run["labels"], tok, run["blank"])
    same_row(run["beam"]["beam"], stats, 4)
    assert run["host_metrics"] == run["plain"] or _nan_equal(run["host_metrics"], run["plain"])
    assert run["beam_host_metrics"] == run["beam"] or _nan_equal(run["beam_host_metrics"], run["beam"])


def _nan_equal(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_nan_equal(a[k], b[k]) for k in a)
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_results_file(run):
    tok = run["model"].tokenizer
    _, greedy_text, refs = host_row(run["greedy"], run["labels"], tok, run["blank"])
    _, beam_text, _ = host_row(run["beam_tokens"], run["labels"], tok, run["blank"])
    lines = open(run["tsv"], encoding="utf-8").read().split("\n")
    assert lines[0] == "PATH\tGROUND_TRUTH\tGREEDY\tBEAM_SEARCH" and lines[-1] == "" and len(lines) == 6  # four utterances, not three
    paths, got_refs, got_greedy, got_beam = M.read_results(run["tsv"])
    assert [os.path.basename(p) for p in paths] == [f"utt{k}.wav" for k in range(4)]  # names default to the entries' paths, file order
    assert got_refs == refs == [tk.normalize_text(t) for t in TEXTS]
    assert got_greedy == greedy_text and got_beam == greedy_text
    paths, got_refs, got_greedy, got_beam = M.read_results(run["tsv_beam"])
    assert paths == ["a", "b", "c", "d"] and got_refs == refs and got_greedy == greedy_text and got_beam == beam_text
    for tsv, res in ((run["tsv"], run["plain"]), (run["tsv_beam"], run["beam"])):
        for where in (None, run["model"].device):
            again = M.evaluate_hypotheses(tsv, device=where)
            for col in ("greedy", "beam"):
                assert _nan_equal(again[col], {k: res[col][k] for k in ("wer", "cer", "mer", "wil", "wip")}), (tsv, where, col)
    ds = run["ds"]
    assert ds.shuffle is True and ds.drop_remainder is True and ds.entries == []  # the dataset object is as it was


def test_oracle_row(run):
    tok, blank = run["model"].tokenizer, run["blank"]
    stats = {u: M.ErrorStats() for u in ("words", "chars", "tokens")}
    beam_words = []
    for (toks, lens, scores), beam, (labels, llen) in zip(run["nbest"], run["beam_tokens"], run["labels"]):
        B, NP = toks.shape[:2]
        ref_text = tok.detokenize(np.stack([np.where(np.arange(labels.shape[1]) < n, row, blank) for row, n in zip(labels, llen)]))
        h, hn, r, rn = M.encode_pairs(tok.detokenize(beam), ref_text, "word")
        beam_words += M.edit_distance_host(h, r, hn, rn).distance.tolist()
        for b in range(B):
            live = [p for p in range(NP) if p == 0 or np.isfinite(scores[b, p])]
            texts = tok.detokenize(np.stack([np.where(np.arange(toks.shape[2]) < lens[b, p], toks[b, p], blank) for p in live]))
            h, hn, r, rn = M.encode_pairs(texts, [ref_text[b]] * len(live), "word")
            words = M.edit_distance_host(h, r, hn, rn)
            best = int(np.argmin(words.distance))  # the first minimum: the lowest index wins a tie
            stats["words"].update(M.EditCounts(*(c[best : best + 1] for c in words)))
            h, hn, r, rn = M.encode_pairs([texts[best]], [ref_text[b]], "char")
            stats["chars"].update(M.edit_distance_host(h, r, hn, rn))
            t, tn = compact(toks[b, live[best]][None, : max(int(lens[b, live[best]]), 0)], blank)
            stats["tokens"].update(M.edit_distance_host(t, labels[b : b + 1], tn, llen[b : b + 1]))
            assert int(words.distance[best]) <= beam_words[len(beam_words) - B + b]  # per utterance: never worse than the beam row
    same_row(run["beam"]["oracle"], stats, 4)
    assert run["beam"]["oracle"]["words"]["distance"] <= run["beam"]["beam"]["words"]["distance"]
    assert _nan_equal(run["beam_host_metrics"]["oracle"], run["beam"]["oracle"])


def test_token_error_rate(run):
    distance = ref = 0
    for toks, (labels, llen) in zip(run["greedy"], run["labels"]):
        h, hn = compact(toks, run["blank"])
        distance += int(M.edit_distance_host(h, labels, hn, llen).distance.sum())
        ref += int(llen.sum())
    assert run["plain"]["greedy"]["ter"] == distance / ref
    assert run["plain"]["greedy"]["tokens"]["ref_length"] == ref
