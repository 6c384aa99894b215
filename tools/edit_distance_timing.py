"""Scoring timing: the device edit distance (kernels.edit_distance) against metrics.edit_distance_host on the same inputs, and where
the time of one model.evaluate batch goes.

Shapes: 32 pairs x ~40 words (WER of one batch), 32 x ~200 characters (CER of one batch), 320 x ~200 characters (an n-best list of 10),
1024 x 512 x 512 (full width, the 8-columns-per-lane wave kernel), and 64 x 2048 x 2048 for the workgroup kernel.  Lengths are ragged
(60 .. 100 % of the width); the hypothesis is the reference with about 15 % of its symbols substituted, dropped or doubled.
Device: HIP events around the call, [median, min, max] ms over --reps after two warm-up calls; inputs already on the device, the counts
stay there.  Host: wall clock around edit_distance_host on the NumPy copies, same statistics over --host-reps.  The outputs of both are
compared.  Nothing existed before this to compare against: the host routine on the same box is the yardstick.

The evaluate split: a tiny random-init Conformer transducer with the character tokenizer, one batch of 32 x 2 s, the three phases of
BaseModel.evaluate timed apart with a device synchronisation after each (wall clock, median of --reps): recognise (greedy search),
detokenise (device -> host copy + tokenizer), score (token, word and character counts; device and host variants).

One process; every step runs under its own time limit (an expired limit writes what exists and ends the process, nothing is retried).

    python tools/edit_distance_timing.py [--out F] [--reps 20] [--host-reps 3]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tensorflowasr_amd import configs  # noqa: E402
from tensorflowasr_amd import kernels as K  # noqa: E402
from tensorflowasr_amd import metrics as M  # noqa: E402
from tensorflowasr_amd import tokenizers as tk  # noqa: E402
from tensorflowasr_amd.conformer import ConformerTransducer  # noqa: E402
from tensorflowasr_amd.schemas import PredictInput  # noqa: E402

RESULT = {}
OUT = [None]


def _expired(signum, frame):
    RESULT["aborted"] = "a step exceeded its time limit"
    _write()
    os._exit(124)


def _write():
    with open(OUT[0], "w") as f:
        json.dump(RESULT, f, indent=1)
        f.write("\n")


class limit:
    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        signal.signal(signal.SIGALRM, _expired)
        signal.alarm(self.seconds)

    def __exit__(self, *a):
        signal.alarm(0)


def stats(ms):
    return [round(float(np.median(ms)), 4), round(float(min(ms)), 4), round(float(max(ms)), 4)]


def pairs(rng, P, width, alphabet):
    ref = rng.integers(0, alphabet, (P, width)).astype(np.int32)
    ref_len = rng.integers(int(0.6 * width), width + 1, P).astype(np.int32)
    hyp = np.zeros((P, width), np.int32)
    hyp_len = np.zeros(P, np.int32)
    for p in range(P):
        out = []
        for s in ref[p, : ref_len[p]]:
            u = rng.random()
            if u < 0.05:
                continue
            out.append(int(rng.integers(0, alphabet)) if u < 0.10 else int(s))
            if u > 0.95:
                out.append(int(s))
        out = out[:width]
        hyp[p, : len(out)], hyp_len[p] = out, len(out)
    return hyp, hyp_len, ref, ref_len


def time_shape(dev, rng, name, P, width, alphabet, reps, host_reps):
    hyp, hyp_len, ref, ref_len = pairs(rng, P, width, alphabet)
    d = [torch.from_numpy(a).to(dev) for a in (hyp, ref, hyp_len, ref_len)]
    for _ in range(2):
        got = K.edit_distance(*d)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got = K.edit_distance(*d)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    host = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        want = M.edit_distance_host(hyp, ref, hyp_len, ref_len)
        host.append((time.perf_counter() - t0) * 1e3)
    same = bool((got.cpu().numpy() == np.stack(want, 1)).all())
    dm, hm = stats(ms), stats(host)
    return dict(shape=name, pairs=P, width=width, alphabet=alphabet, device_ms=dm, host_ms=hm, host_over_device=round(hm[0] / dm[0], 1),
                outputs_equal=same, mean_distance=round(float(np.mean(want.distance)), 1))


def evaluate_split(dev, reps):
    vocab = os.path.join(ROOT, "tests", "golden", "librispeech", "characters", "english.vocab")
    tok = tk.get({"type": "characters", "blank_index": 0, "vocabulary": vocab})
    model = ConformerTransducer(configs.conformer_tiny(vocab_size=tok.num_classes), dev, dtype=torch.float32, seed=3)
    model.tokenizer = tok
    rng = np.random.default_rng(2)
    B, n, U = 32, 32000, 30
    sig = torch.from_numpy(np.clip(rng.standard_normal((B, n)) * 0.1, -1, 1).astype(np.float32)).to(dev)
    inp = PredictInput(sig, torch.full((B,), n, dtype=torch.int32), model.get_initial_tokens(batch_size=B), None,
                       model.get_initial_decoder_states(batch_size=B))
    labels = torch.from_numpy(rng.integers(1, tok.num_classes, (B, U)).astype(np.int32)).to(dev)
    llen = torch.from_numpy(rng.integers(U // 2, U + 1, B).astype(np.int32)).to(dev)
    refs = tok.detokenize(labels.cpu().numpy())

    def sync_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def score(tokens, texts, device):
        where = dev if device else None
        if device:
            M.edit_distance(tokens, labels, None, llen, model.blank)
        else:
            M.edit_distance(tokens.cpu(), labels.cpu(), None, llen.cpu(), model.blank)
        words = M.score_texts(texts, refs, "word", where)
        chars = M.score_texts(texts, refs, "char", where)
        return int(words.distance.sum()), int(chars.distance.sum())  # reading the sums is the synchronisation a caller pays

    rec, det, sc_dev, sc_host = [], [], [], []
    for k in range(reps + 2):
        t_rec, tokens = sync_ms(lambda: model.recognize(inp).tokens.to(torch.int32).contiguous())
        t_det, texts = sync_ms(lambda: tok.detokenize(tokens.cpu().numpy()))
        t_dev, a = sync_ms(lambda: score(tokens, texts, True))
        t_host, b = sync_ms(lambda: score(tokens, texts, False))
        assert a == b
        if k >= 2:
            rec.append(t_rec), det.append(t_det), sc_dev.append(t_dev), sc_host.append(t_host)
    ntok = int(((tokens >= 0) & (tokens != model.blank)).sum())
    return dict(model="conformer_tiny f32, characters (V = 29), random weights", batch=B, seconds=n / 16000, hypothesis_tokens=ntok,
                hypothesis_width=int(tokens.shape[1]), recognise_ms=stats(rec), detokenise_ms=stats(det), score_device_ms=stats(sc_dev),
                score_host_ms=stats(sc_host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_distance_timing.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    OUT[0] = a.out
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    RESULT.update(device=torch.cuda.get_device_name(0), reps=a.reps, host_reps=a.host_reps,
                  note="[median, min, max] ms; device = HIP events around kernels.edit_distance, host = wall clock around "
                       "metrics.edit_distance_host on the same inputs; measured once", shapes=[])
    for name, P, width, alphabet, seconds in (("32 x 40 words", 32, 40, 5000, 60), ("32 x 200 chars", 32, 200, 28, 60),
                                              ("320 x 200 chars (n-best 10)", 320, 200, 28, 60), ("1024 x 512 x 512", 1024, 512, 28, 240),
                                              ("64 x 2048 x 2048 (workgroup kernel)", 64, 2048, 28, 240)):
        with limit(seconds):
            RESULT["shapes"].append(time_shape(dev, rng, name, P, width, alphabet, a.reps, a.host_reps))
        _write()
    with limit(180):
        RESULT["evaluate_batch"] = evaluate_split(dev, min(a.reps, 10))
    _write()
    print(json.dumps(RESULT, indent=1))


if __name__ == "__main__":
    main()
