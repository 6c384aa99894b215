"""Scoring transcripts: word / character / token error rates from batched edit distances, and the results `.tsv`.

What the reference does with jiwer and tf.edit_distance (scripts/test.py, callbacks.PredictLogger / TestLogger, metrics/error_rates.py,
utils/app_util.evaluate_hypotheses), on arithmetic of this package: the device routine is csrc/edit_distance.hip (kernels.edit_distance),
`edit_distance_host` is the same definition in NumPy and serves CPU inputs and pairs wider than TFASR_EDIT_MAX_LEN.

Definition.  A pair scores a hypothesis against a reference with unit costs.  `distance` is unique; hits / substitutions / deletions /
insertions are not (for "a b" against "b a" both {2 substitutions} and {1 hit, 1 deletion, 1 insertion} cost 2).  The counts returned are
those of the minimum-distance alignment with the MOST hits, which is also the one with the fewest substitutions.  WER, CER and the token
error rate depend on the distance only.  MER / WIL / WIP depend on the counts, so on such ties they may differ from jiwer's, whose
back-trace preference is not reproduced here [ext: the library is not available to compare against].

Rates (ErrorStats), jiwer's corpus-level definitions [ext], over the sums of all pairs seen:
    wer = (S+D+I) / (H+S+D)      mer = (S+D+I) / (H+S+D+I)      wip = (H / N_ref) * (H / N_hyp), 0 when N_hyp = 0      wil = 1 - wip
A zero denominator gives nan (np.divide in TestLogger.on_test_end).  An utterance with an empty reference adds its insertions to the
sums and nothing to the denominator: it cannot divide by zero on its own (jiwer raises on an empty reference).
"""
import math
import typing

import numpy as np
import torch

EDIT_MAX_LEN = 4096  # TFASR_EDIT_MAX_LEN (include/tfasr_hip.h)
TSV_HEADER = ("PATH", "GROUND_TRUTH", "GREEDY", "BEAM_SEARCH")


class EditCounts(typing.NamedTuple):
    """[P] int32 each (torch tensors from `edit_distance`, NumPy arrays from `edit_distance_host`)."""
    distance: typing.Any
    hits: typing.Any
    substitutions: typing.Any
    deletions: typing.Any
    insertions: typing.Any


# ------------------------------------------------------------------------------------------------------ edit distance
def _sequences(rows, lens, skip_id):
    """rows [P, W] (+ lengths, or None: drop entries < 0 and == skip_id) -> (left-packed int64 [P, W'], lengths [P] int64)"""
    rows = np.asarray(rows)
    if rows.ndim != 2:
        raise ValueError("sequences must be [P, width]")
    rows = rows.astype(np.int64)
    P, W = rows.shape
    if lens is not None:
        n = np.clip(np.asarray(lens).astype(np.int64).reshape(P), 0, W)
        return rows, n
    keep = rows >= 0
    if skip_id is not None:
        keep &= rows != int(skip_id)
    n = keep.sum(1)
    out = np.zeros((P, max(int(n.max()) if P else 0, 1)), np.int64)
    pos = np.cumsum(keep, 1) - 1
    r, c = np.nonzero(keep)
    out[r, pos[r, c]] = rows[r, c]
    return out, n


def edit_distance_host(hyp, ref, hyp_len=None, ref_len=None, skip_id=None) -> EditCounts:
    """The definition of the module docstring in NumPy, for any width.  One pass over the hypothesis positions, every pair and every
    reference column at once: the value is dist * BIG - hits; substitution / hit and insertion come from the previous row, and the
    in-row dependency of the deletions (v[k] = min(c[k], v[k-1] + BIG)) is a running minimum of c[k] - k * BIG."""
    h, n = _sequences(hyp, hyp_len, skip_id)
    r, m = _sequences(ref, ref_len, skip_id)
    if h.shape[0] != r.shape[0]:
        raise ValueError("hyp and ref must hold the same number of pairs")
    P = h.shape[0]
    BIG = np.int64(1) << 32
    M = int(m.max()) if P else 0
    r = r[:, :M]
    ramp = np.arange(M + 1, dtype=np.int64) * BIG
    v = np.broadcast_to(ramp, (P, M + 1)).copy()  # row 0
    for i in range(int(n.max()) if P else 0):
        c = np.empty_like(v)
        c[:, 0] = (i + 1) * BIG
        np.minimum(v[:, :-1] + np.where(h[:, i : i + 1] == r, np.int64(-1), BIG), v[:, 1:] + BIG, out=c[:, 1:])
        c = np.minimum.accumulate(c - ramp, axis=1) + ramp
        live = i < n
        v[live] = c[live]
    val = v[np.arange(P), m] if P else np.zeros(0, np.int64)
    d = (val + BIG - 1) >> 32
    hits = d * BIG - val
    ins = d - (m - hits)
    dele = ins + m - n
    sub = m - hits - dele
    return EditCounts(*(x.astype(np.int32) for x in (d, hits, sub, dele, ins)))


def edit_distance(hyp, ref, hyp_len=None, ref_len=None, skip_id=None) -> EditCounts:
    """Edit distance and counts of P pairs, hyp [P, N] against ref [P, M].  A side with lengths uses its first len entries; a side
    without is compacted (entries < 0 and entries == skip_id dropped, the blank-padded output of the searches).  Device tensors go to
    the HIP kernel; NumPy arrays, CPU tensors and pairs wider than TFASR_EDIT_MAX_LEN go to edit_distance_host.  -> EditCounts of
    [P] int32 tensors on the inputs' device."""
    on_device = isinstance(hyp, torch.Tensor) and hyp.is_cuda
    if on_device and hyp.shape[1] <= EDIT_MAX_LEN and ref.shape[1] <= EDIT_MAX_LEN:
        from . import kernels as K

        i32 = lambda t: None if t is None else t.to(hyp.device).to(torch.int32).contiguous()
        counts = K.edit_distance(i32(hyp), i32(ref), i32(hyp_len), i32(ref_len), -1 if skip_id is None else int(skip_id))
        return EditCounts(*counts.unbind(1))
    host = lambda t: None if t is None else (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t))
    out = edit_distance_host(host(hyp), host(ref), host(hyp_len), host(ref_len), skip_id)
    dev = hyp.device if isinstance(hyp, torch.Tensor) else torch.device("cpu")
    return EditCounts(*(torch.from_numpy(x).to(dev) for x in out))


# ------------------------------------------------------------------------------------------------------ text -> symbols
def encode_pairs(hyps, refs, unit="word"):
    """Two equally long lists of strings -> (hyp [P, L] int32, hyp_len [P], ref [P, L'] int32, ref_len [P]) NumPy arrays, zero padded.
    unit "word": str.split() pieces (runs of white space collapse), interned over BOTH lists of the call - what tf.strings.split and
    jiwer's default word transform amount to; "char": code points of the stripped string, inner spaces kept (jiwer.process_characters);
    "byte": UTF-8 bytes (TestLogger.compute_cer's bytes_split)."""
    hyps, refs = list(hyps), list(refs)
    if len(hyps) != len(refs):
        raise ValueError("hyps and refs must hold the same number of transcripts")
    if unit == "word":
        ids = {}
        enc = lambda s: [ids.setdefault(w, len(ids)) for w in s.split()]
    elif unit == "char":
        enc = lambda s: [ord(ch) for ch in s.strip()]
    elif unit == "byte":
        enc = lambda s: list(s.encode("utf-8"))
    else:
        raise ValueError(f"unit must be 'word', 'char' or 'byte', not {unit!r}")

    def pad(seqs):
        n = np.asarray([len(s) for s in seqs], np.int32).reshape(len(seqs))
        out = np.zeros((len(seqs), max(int(n.max()) if len(seqs) else 0, 1)), np.int32)
        for k, s in enumerate(seqs):
            out[k, : len(s)] = s
        return out, n

    h, hn = pad([enc(s) for s in hyps])
    r, rn = pad([enc(s) for s in refs])
    return h, hn, r, rn


def score_texts(hyps, refs, unit="word", device=None) -> EditCounts:
    """Counts of every (hypothesis, reference) transcript pair; on `device` when given, else on the host."""
    h, hn, r, rn = encode_pairs(hyps, refs, unit)
    if device is None:
        return edit_distance(h, r, hn, rn)
    dev = torch.device(device)
    return edit_distance(*(torch.from_numpy(x).to(dev) for x in (h, r, hn, rn)))


# ------------------------------------------------------------------------------------------------------ accumulator
def _div(a, b):
    return a / b if b else math.nan


class ErrorStats:
    """Sums of the counts over every pair added (the numerator / denominator idea of the reference's ErrorRate metric)."""

    FIELDS = ("distance", "hits", "substitutions", "deletions", "insertions", "hyp_length", "ref_length", "pairs")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, 0)

    def update(self, counts: EditCounts):
        d, h, s, dl, i = (np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x).astype(np.int64) for x in counts)
        self.distance += int(d.sum())
        self.hits += int(h.sum())
        self.substitutions += int(s.sum())
        self.deletions += int(dl.sum())
        self.insertions += int(i.sum())
        self.hyp_length += int((h + s + i).sum())
        self.ref_length += int((h + s + dl).sum())
        self.pairs += int(d.size)
        return self

    @property
    def error_rate(self):
        """(S+D+I) / N_ref: WER for words, CER for characters or bytes, token error rate for tokens."""
        return _div(self.distance, self.ref_length)

    wer = error_rate

    @property
    def mer(self):
        return _div(self.distance, self.hits + self.distance)

    @property
    def wip(self):
        if self.ref_length == 0:
            return math.nan
        return (self.hits / self.ref_length) * (self.hits / self.hyp_length) if self.hyp_length else 0.0

    @property
    def wil(self):
        return 1.0 - self.wip

    def counts(self):
        return {f: getattr(self, f) for f in self.FIELDS}


def summary(words: ErrorStats, chars: ErrorStats):
    return {"wer": words.wer, "cer": chars.error_rate, "mer": words.mer, "wil": words.wil, "wip": words.wip}


# ------------------------------------------------------------------------------------------------------ results file
class ResultsWriter:
    """The results file of PredictLogger: a header, then PATH<TAB>GROUND_TRUTH<TAB>GREEDY<TAB>BEAM_SEARCH per utterance."""

    def __init__(self, filepath):
        self.file = open(filepath, "w", encoding="utf-8")
        self.file.write("\t".join(TSV_HEADER) + "\n")

    def write(self, paths, references, greedy, beam):
        for fields in zip(paths, references, greedy, beam):
            self.file.write("\t".join(" ".join(str(f).split("\t")).replace("\n", " ") for f in fields) + "\n")

    def close(self):
        self.file.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_results(filepath):
    """-> (paths, references, greedy hypotheses, beam hypotheses) of a results file"""
    cols = ([], [], [], [])
    with open(filepath, "r", encoding="utf-8") as f:
        lines = f.read().split("\n")
    for ln in lines[1:]:
        if not ln:
            continue
        parts = ln.split("\t")
        if len(parts) != 4:
            raise ValueError(f"{filepath}: expected {' '.join(TSV_HEADER)} separated by tabs, got {ln!r}")
        for c, p in zip(cols, parts):
            c.append(p)
    return cols


def evaluate_hypotheses(filepath, device=None, cer_unit="char"):
    """utils/app_util.evaluate_hypotheses: {"greedy": {wer, cer, mer, wil, wip}, "beam": {...}} of a results file, NOT multiplied by 100,
    as a plain dict.  Scored on `device` when given (a HIP device), else on the host; the numbers are the same."""
    _, refs, greedy, beam = read_results(filepath)
    out = {}
    for name, hyps in (("greedy", greedy), ("beam", beam)):
        words = ErrorStats().update(score_texts(hyps, refs, "word", device))
        chars = ErrorStats().update(score_texts(hyps, refs, cer_unit, device))
        out[name] = summary(words, chars)
    return out
