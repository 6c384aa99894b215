"""Commit horizon and trie compaction of the beam streams, timing (recorded, no pass / fail bar).  Three measurements, each alternated
with the call it is compared to in one run, medians of synchronised wall times:

  commit      K.CtcBeamStream / K.RnntBeamStream.commit(horizon=H) against commit() on the same carried beams, B = 1 and 32, W = 10,
              V = 1000, after 48 frames in chunks of 16 (H = 16: every call after the second is a prune point with a point in reach)
  compact     one compact() of streams whose tries are nearly full: W = 10, V = 1000, Tcap = 3000, 2990 frames consumed, committed by
              a plain commit first (CTC; B = 1 and 32), with the nodes kept; and again right after (nothing left to drop)
  session     a whole session step (accept of one chunk of audio), Conformer-S streaming config of tools/stream_beam_timing.py, W = 10,
              B = 1 and 32, with commit_horizon = 16 (max_frames = 64: the session compacts every few chunks) against the plain beam session

One process; every step runs under its own time limit (an expired limit writes what exists and ends the process, nothing is retried).
Output: profiles/stream_horizon_timing.json (default).

    python tools/stream_horizon_timing.py [--out F] [--seconds 10] [--batches 1,32] [--reps 20]
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tensorflowasr_amd import configs  # noqa: E402
from tensorflowasr_amd import kernels as K  # noqa: E402
from tensorflowasr_amd.conformer import ConformerTransducer  # noqa: E402

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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def quiet_loud(rng, B, T, V):
    """logits [B, T, V] f32, blank V - 1: 75 % of the frames N(0,1) * 0.5 with +8 on the blank, the rest N(0,1) * 2"""
    x = rng.standard_normal((B, T, V))
    q = rng.random((B, T)) < 0.75
    x = np.where(q[..., None], x * 0.5, x * 2.0)
    x[..., V - 1] += 8.0 * q
    return torch.from_numpy(x.astype(np.float32))


def rnnt_weights(dev, V, E, U, J):
    g = torch.Generator().manual_seed(0)
    r = lambda *s, fan: (torch.randn(*s, generator=g) / fan ** 0.5).to(dev)
    return (r(V, E, fan=1), r(E, 4 * U, fan=E), r(U, 4 * U, fan=U), r(4 * U, fan=4), None, None, r(U, J, fan=U), r(J, fan=4),
            r(J, V, fan=J / 9), r(V, fan=1))


def commit_timing(dev, B, reps):
    V, W, C, H = 1000, 10, 16, 16
    rng = np.random.default_rng(B)
    out = {}
    x = quiet_loud(rng, B, 3 * C, V).to(dev)
    w = rnnt_weights(dev, V, 64, 64, 64)
    encj = torch.randn(B, 3 * C, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    for head in ("ctc", "transducer"):
        plain_t, hor_t = [], []
        for _ in range(reps):
            pair = []
            for _ in range(2):
                pair.append(K.CtcBeamStream(B, C, 4 * C, V, W, device=dev) if head == "ctc" else K.RnntBeamStream(w, B, 4 * C, W))
            for i in range(3):
                for k, s in enumerate(pair):
                    s.advance((x if head == "ctc" else encj)[:, i * C:(i + 1) * C].contiguous(), [C] * B)
                    t = timed((lambda: s.commit(horizon=H)) if k else s.commit)
                    if i == 2:
                        (hor_t if k else plain_t).append(t)
        out[head] = dict(plain_commit_ms_median=statistics.median(plain_t), horizon_commit_ms_median=statistics.median(hor_t))
    return out


def compact_timing(dev, B, reps):
    V, W, C, Tcap, T = 1000, 10, 230, 3000, 2990
    x = quiet_loud(np.random.default_rng(100 + B), B, T, V).to(dev)
    first, again, twin_commit = [], [], []
    kept = None
    for _ in range(max(reps // 4, 2)):
        s = K.CtcBeamStream(B, C, Tcap, V, W, device=dev)
        for t0 in range(0, T, C):
            s.advance(x[:, t0:t0 + C].contiguous(), [C] * B)
        twin_commit.append(timed(s.commit))
        res = []
        first.append(timed(lambda: res.append(s.compact())))
        kept = [r[1] for r in res[0]]
        again.append(timed(s.compact))
    return dict(frames=T, nodes_before_at_most=1 + W * T, nodes_kept=kept, compact_ms_median=statistics.median(first),
                compact_again_ms_median=statistics.median(again), plain_commit_ms_median=statistics.median(twin_commit))


def session_once(model, sig, chunk, W, max_frames, horizon):
    B, n = sig.shape
    rec = model.stream_horizon(horizon, B, precision="f32", beam_width=W, max_frames=max_frames) if horizon else \
        model.stream(B, precision="f32", beam_width=W, max_frames=max_frames)
    times, ntok = [], 0
    for p0 in range(0, n, chunk):
        c0 = rec.chunks_run
        x = torch.from_numpy(sig[:, p0:p0 + chunk])
        res = []
        t = timed(lambda: res.append(rec.accept(x)))
        if rec.chunks_run == c0 + 1:
            times.append(t)
        ntok += int(res[0].tokens_length.sum())
    ntok += int(rec.finish().tokens_length.sum())
    return times, ntok, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_horizon_timing.json"))
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    OUT[0] = a.out
    dev = torch.device("cuda:0")
    batches = [int(v) for v in a.batches.split(",")]
    RESULT.update(device=torch.cuda.get_device_name(0), note="measured once; medians of synchronised wall times, the compared calls alternate",
                  commit=[], compact=[], session=[])
    for B in batches:
        with limit(300):
            commit_timing(dev, B, 2)  # warm-up
            RESULT["commit"].append(dict(B=B, W=10, V=1000, horizon=16, **commit_timing(dev, B, a.reps)))
        _write()
    for B in batches:
        with limit(300):
            RESULT["compact"].append(dict(B=B, W=10, V=1000, Tcap=3000, **compact_timing(dev, B, a.reps)))
        _write()
    cfg = configs.conformer_s(vocab_size=1000, chunk_size=16, history_size=64, convm_dw_norm="layer", sub_norm="layer", dropout=0.0)
    cfg.time_masking, cfg.freq_masking = {}, {}
    chunk = 640 * cfg.chunk_size
    with limit(120):
        model = ConformerTransducer(cfg, dev, dtype=torch.bfloat16, seed=0)
        model.ps.p("joint/vocab/b")[0] += 0.7  # (random weights never emit the blank otherwise)
    rng = np.random.default_rng(0)
    W, H = 10, 16
    plain_frames = int(a.seconds * 25) + cfg.chunk_size
    for B in batches:
        sig = np.clip(rng.standard_normal((B, int(a.seconds * 16000))) * 0.1, -1, 1).astype(np.float32)
        with limit(300):
            session_once(model, sig, chunk, W, plain_frames, None)
            session_once(model, sig, chunk, W, 64, H)
        pt, ht, r = [], [], dict(B=B, beam_width=W, commit_horizon=H, horizon_max_frames=64, plain_max_frames=plain_frames,
                                 chunk_audio_ms=cfg.chunk_size * 40.0)
        for _ in range(2):
            with limit(300):
                t, ntok, _ = session_once(model, sig, chunk, W, plain_frames, None)
                pt += t
                r["plain_tokens"] = ntok
            with limit(300):
                t, ntok, rec = session_once(model, sig, chunk, W, 64, H)
                ht += t
                r["horizon_tokens"] = ntok
                r["labels_dropped_by_compactions"] = sum(len(d) for d in rec.beam.dropped)
        r.update(plain_chunk_ms_median=statistics.median(pt), plain_chunk_ms_worst=max(pt), horizon_chunk_ms_median=statistics.median(ht),
                 horizon_chunk_ms_worst=max(ht))
        RESULT["session"].append(r)
        _write()
    print(json.dumps(RESULT))
    _write()


if __name__ == "__main__":
    main()
