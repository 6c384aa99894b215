"""Streaming recognition timing: Conformer-S streaming config (chunk 16, history 64, V = 1000), 10 s of audio per stream, B = 1 and
B = 32, f32 and bf16 encoder.  Per configuration: the synchronised time of every `accept` of one chunk of audio (median and worst over
the utterance, after a warm-up utterance), kernel launches per chunk, the whole streamed utterance, and the offline `recognize` of the
same audio in the same run (B > 1: recognize_batch's rule, so its tokens are not the session's; the time is what is compared).

One process; every step runs under its own time limit (an expired limit writes what exists and ends the process, nothing is retried).
Output: profiles/stream_timing.json (default) - a chunk is chunk_size * 40 ms of audio, so `chunk_ms_median` at B = 1 at or above
`chunk_audio_ms` would mean the session cannot keep up with a microphone.

    python tools/stream_timing.py [--out F] [--seconds 10] [--batches 1,32]
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


def stream_once(model, sig, chunk, precision, timed):
    """one utterance through a session, `chunk` samples per accept; -> (per-accept ms, launches per accept that ran a chunk, total ms, tokens)"""
    B, n = sig.shape
    rec = model.stream(B, precision=precision)
    times, launches, ntok = [], [], 0
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for p0 in range(0, n, chunk):
        x = torch.from_numpy(sig[:, p0:p0 + chunk])
        l0, c0 = K.launch_count(), rec.chunks_run
        t0 = time.perf_counter()
        out = rec.accept(x)
        torch.cuda.synchronize()
        if timed and rec.chunks_run == c0 + 1:
            times.append((time.perf_counter() - t0) * 1e3)
            launches.append(K.launch_count() - l0)
        ntok += int(out.tokens_length.sum())
    out = rec.finish()
    torch.cuda.synchronize()
    ntok += int(out.tokens_length.sum())
    return times, launches, (time.perf_counter() - t_all) * 1e3, ntok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_timing.json"))
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--batches", default="1,32")
    a = ap.parse_args()
    OUT[0] = a.out
    dev = torch.device("cuda:0")
    cfg = configs.conformer_s(vocab_size=1000, chunk_size=16, history_size=64, convm_dw_norm="layer", sub_norm="layer", dropout=0.0)
    cfg.time_masking, cfg.freq_masking = {}, {}
    chunk = 640 * cfg.chunk_size  # samples of one chunk of audio
    RESULT.update(model="Conformer-S streaming (chunk 16, history 64, 16 blocks, V = 1000, random weights)", seconds=a.seconds,
                  chunk_audio_ms=cfg.chunk_size * 40.0, device=torch.cuda.get_device_name(0), runs=[])
    with limit(120):
        model = ConformerTransducer(cfg, dev, dtype=torch.bfloat16, seed=0)
        model.ps.p("joint/vocab/b")[0] += 0.7  # (random weights never emit the blank otherwise: 3 symbols on every frame)
    rng = np.random.default_rng(0)
    for B in [int(v) for v in a.batches.split(",")]:
        sig = np.clip(rng.standard_normal((B, int(a.seconds * 16000))) * 0.1, -1, 1).astype(np.float32)
        for precision in ("f32", "bf16"):
            r = dict(B=B, precision=precision)
            with limit(240):
                stream_once(model, sig, chunk, precision, False)  # warm-up utterance (workspaces, packed search weights, allocator)
            with limit(240):
                times, launches, total, ntok = stream_once(model, sig, chunk, precision, True)
            r.update(chunks=len(times), chunk_ms_median=statistics.median(times), chunk_ms_worst=max(times), chunk_ms_best=min(times),
                     launches_per_chunk_median=statistics.median(launches), launches_per_chunk_max=max(launches), streamed_total_ms=total,
                     tokens=ntok)
            inp = PredictInput(torch.from_numpy(sig), torch.tensor([sig.shape[1]] * B))
            with limit(240):
                model.recognize(inp, precision=precision)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.recognize(inp, precision=precision)
                torch.cuda.synchronize()
                r["offline_recognize_ms"] = (time.perf_counter() - t0) * 1e3
            r["streamed_over_offline"] = r["streamed_total_ms"] / r["offline_recognize_ms"]
            r["keeps_up_with_a_microphone"] = r["chunk_ms_worst"] < RESULT["chunk_audio_ms"]
            RESULT["runs"].append(r)
            print(json.dumps(r), flush=True)
            _write()
    _write()


if __name__ == "__main__":
    main()
