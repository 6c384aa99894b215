"""N-gram LM fusion in the carried CTC beam (K.CtcLmBeamStream, tfasr_ctc_beam_lm_*) against the plain carried beam (K.CtcBeamStream),
timing (recorded, no pass / fail bar).  The two shapes of profiles/ctc_lm_beam_timing.json - V = 1000 / W = 10 / order 3 and V = 29 /
W = 32 / order 5, NGramLM.estimate over seeded Markov-chain sequences, blank 0 for both streams - on two kinds of logits: seeded random
(x 3), and the quiet / loud logits of tests/beam_horizon_oracle.py (75 % of the frames near-certain blanks), which are closer to a
model's.  Every fused call alternates with the plain call it is compared to in one run; [median, min, max] ms of HIP events around one
call:

  advance     one advance of a 16-frame chunk, fused / fused at zero weights (the plain search's hypotheses found the fused way) /
              plain, B = 1 and 32, the streams 32 to 250 frames into their utterances
  commit      commit() right after each of those advances, fused against plain
  compact     one compact() of streams whose tries are nearly full (Tcap = 3000, 2990 frames consumed, a plain commit first), fused
              against plain, with the nodes kept
  utterance   a whole utterance of 250 frames in 16-frame chunks (reset + 16 advances + n-best) against the one-shot fused search
              (tfasr_ctc_beam_search_lm) on the same logits, B = 1 and 32; whether the two n-best lists are bit-equal

One process; every step runs under its own time limit (an expired limit writes what exists and ends the process, nothing is retried).

    python tools/ctc_lm_stream_timing.py [--out profiles/ctc_lm_stream_timing.json] [--batches 1,32] [--reps 3]
"""
import argparse
import json
import os
import signal
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tensorflowasr_amd import kernels as K  # noqa: E402
from tensorflowasr_amd.lm import NGramLM  # noqa: E402

SHAPES = [dict(V=1000, W=10, order=3), dict(V=29, W=32, order=5)]
ALPHA, BETA = 0.5, 0.1
C, T = 16, 250
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
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return [round(float(np.median(ms)), 4), round(float(min(ms)), 4), round(float(max(ms)), 4)]


def slower(fused, plain):
    """is the fused median above the plain one by more than the plain call's own run-to-run spread (max - min)?"""
    return bool(fused[0] - plain[0] > plain[2] - plain[1])


def markov_sequences(V, n, seed):  # tools/ctc_lm_beam_timing.py's
    rng = np.random.default_rng(seed)
    fav = rng.integers(1, V, size=(V, 3))
    out = []
    for _ in range(n):
        cur, s = int(rng.integers(1, V)), []
        for _ in range(int(rng.integers(5, 40))):
            s.append(cur)
            cur = int(fav[cur, rng.integers(3)]) if rng.random() < 0.8 else int(rng.integers(1, V))
        out.append(s)
    return out


def make_logits(kind, rng, B, frames, V):
    """blank 0.  "random": N(0,1) * 3; "quiet_loud": tests/beam_horizon_oracle.py's rule"""
    x = rng.standard_normal((B, frames, V))
    if kind == "random":
        return torch.from_numpy((x * 3.0).astype(np.float32))
    q = rng.random((B, frames)) < 0.75
    x = np.where(q[..., None], x * 0.5, x * 2.0)
    x[..., 0] += 8.0 * q
    return torch.from_numpy(x.astype(np.float32))


def chunks(x):
    return [x[:, t0:t0 + C].contiguous() for t0 in range(0, x.shape[1], C)]


def advance_commit(dev, B, V, W, tables, zero, x, reps):
    """per repetition three fresh streams walk the utterance together, chunk by chunk; the chunks from frame 32 on are timed"""
    t = {k: [] for k in ("fused_advance", "zero_advance", "plain_advance", "fused_commit", "plain_commit")}
    xs = chunks(x)
    for _ in range(reps):
        f = K.CtcLmBeamStream(B, C, T + C, V, W, tables, blank_index=0, device=dev)
        z = K.CtcLmBeamStream(B, C, T + C, V, W, zero, blank_index=0, device=dev)
        p = K.CtcBeamStream(B, C, T + C, V, W, blank_index=0, device=dev)
        for i, xc in enumerate(xs):
            nv = [xc.shape[1]] * B
            took = [timed(lambda s=s: s.advance(xc, nv)) for s in (f, z, p)]
            com = [timed(s.commit) for s in (f, p)]
            if i >= 2 and xc.shape[1] == C:
                for k, v in zip(("fused_advance", "zero_advance", "plain_advance"), took):
                    t[k].append(v)
                t["fused_commit"].append(com[0])
                t["plain_commit"].append(com[1])
    r = {k + "_ms": stats(v) for k, v in t.items()}
    r["fused_over_plain_advance"] = round(r["fused_advance_ms"][0] / r["plain_advance_ms"][0], 2)
    r["zero_weights_over_plain_advance"] = round(r["zero_advance_ms"][0] / r["plain_advance_ms"][0], 2)
    r["fused_over_plain_commit"] = round(r["fused_commit_ms"][0] / r["plain_commit_ms"][0], 2)
    r["fused_advance_slower_than_plain_spread"] = slower(r["fused_advance_ms"], r["plain_advance_ms"])
    r["zero_advance_slower_than_plain_spread"] = slower(r["zero_advance_ms"], r["plain_advance_ms"])
    r["fused_commit_slower_than_plain_spread"] = slower(r["fused_commit_ms"], r["plain_commit_ms"])
    return r


def utterance(dev, B, V, W, tables, x, reps):
    ln = torch.full((B,), T, dtype=torch.int32, device=dev)
    xs = chunks(x)
    s = K.CtcLmBeamStream(B, C, T, V, W, tables, blank_index=0, device=dev)
    got = []

    def in_chunks():
        s.reset()
        for xc in xs:
            s.advance(xc, [xc.shape[1]] * B)
        got[:] = s.nbest(1, final_rows=range(B))

    one, piece = [], []
    for i in range(reps + 1):
        a = timed(lambda: got.__setitem__(slice(None), K.ctc_beam_search_lm(x, ln, tables, beam_width=W, top_paths=1, blank_index=0)))
        want = [v.clone() for v in got]
        b = timed(in_chunks)
        if i:  # (the first round warms up)
            one.append(a)
            piece.append(b)
    same = all(torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
               for u, v in zip(got, want))
    r = dict(one_shot_ms=stats(one), chunked_ms=stats(piece), chunks=len(xs), outputs_bit_equal=bool(same),
             mean_tokens=round(float(got[1][:, 0].float().mean()), 1))
    r["chunked_over_one_shot"] = round(r["chunked_ms"][0] / r["one_shot_ms"][0], 2)
    return r


def compact(dev, B, V, W, tables, kind, reps):
    Tcap, frames, step = 3000, 2990, 230
    x = make_logits(kind, np.random.default_rng(100 + B + V), B, frames, V).to(dev)
    t = {"fused": [], "plain": []}
    kept = {}
    for _ in range(reps):
        pair = {"fused": K.CtcLmBeamStream(B, step, Tcap, V, W, tables, blank_index=0, device=dev),
                "plain": K.CtcBeamStream(B, step, Tcap, V, W, blank_index=0, device=dev)}
        for t0 in range(0, frames, step):
            for s in pair.values():
                s.advance(x[:, t0:t0 + step].contiguous(), [step] * B)
        for who, s in pair.items():
            s.commit()
            res = []
            t[who].append(timed(lambda: res.append(s.compact())))
            kept[who] = [r[1] for r in res[0]][:4]
    r = dict(frames=frames, nodes_before_at_most=1 + W * frames, nodes_kept_first_streams=kept, fused_compact_ms=stats(t["fused"]),
             plain_compact_ms=stats(t["plain"]), note="compact() reads its result back: one device-to-host copy is in both times")
    r["fused_over_plain_compact"] = round(r["fused_compact_ms"][0] / r["plain_compact_ms"][0], 2)
    r["fused_compact_slower_than_plain_spread"] = slower(r["fused_compact_ms"], r["plain_compact_ms"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_lm_stream_timing.json"))
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctc_lm_stream_timing: no GPU (timings are taken on the device only)")
    OUT[0] = a.out
    dev = torch.device("cuda:0")
    batches = [int(v) for v in a.batches.split(",")]
    RESULT.update(device=torch.cuda.get_device_name(0), alpha_beta=[ALPHA, BETA], chunk_frames=C, utterance_frames=T,
                  note="measured once; [median, min, max] ms, HIP events around one call, fused and plain calls alternate; "
                       "*_slower_than_plain_spread: the fused median exceeds the plain median by more than the plain call's max - min",
                  rows=[])
    for sh in SHAPES:
        V, W, order = sh["V"], sh["W"], sh["order"]
        lm = NGramLM.estimate(markov_sequences(V, 400, V), order, V, 0)
        tables, zero = lm.tables(ALPHA, BETA), lm.tables(0.0, 0.0)
        for kind in ("random", "quiet_loud"):
            for B in batches:
                row = dict(sh, logits=kind, B=B, lm_nodes=tables.nodes)
                x = make_logits(kind, np.random.default_rng(V + B), B, T, V).to(dev)
                with limit(240):
                    advance_commit(dev, B, V, W, tables, zero, x, 1)  # warm-up
                    row.update(advance_commit(dev, B, V, W, tables, zero, x, a.reps))
                with limit(240):
                    row["utterance"] = utterance(dev, B, V, W, tables, x, a.reps)
                with limit(300):
                    row["compact"] = compact(dev, B, V, W, tables, kind, max(a.reps, 3))
                RESULT["rows"].append(row)
                print(json.dumps(row), flush=True)
                _write()
    _write()


if __name__ == "__main__":
    main()
