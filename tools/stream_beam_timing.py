"""Beam search in streaming sessions, timing: Conformer-S streaming config (chunk 16, history 64, V = 1000), 10 s of audio per stream,
B = 1 and B = 32, beam_width 4 and 10, f32.  Per configuration: the synchronised time of every `accept` of one chunk of audio (median
and worst over the utterance, after a warm-up utterance) and the kernel launches per chunk, for the beam session and for the greedy
session on the same audio in the same run (the two alternate, utterance by utterance), and `recognize_beam_encoded` over the frames the
beam session logged (the offline search of the same frames; its n-best must equal the session's bit for bit, which is recorded).

One process; every step runs under its own time limit (an expired limit writes what exists and ends the process, nothing is retried).
Output: profiles/stream_beam_timing.json (default).  A chunk is chunk_size * 40 ms of audio: `chunk_ms_median` at B = 1 at or above
`chunk_audio_ms` would mean the session cannot keep up with a microphone.

    python tools/stream_beam_timing.py [--out F] [--seconds 10] [--batches 1,32] [--widths 4,10] [--rounds 2]
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


def stream_once(model, sig, chunk, beam_width, max_frames, log=False):
    """one utterance through a session, `chunk` samples per accept -> (per-accept ms, launches per accept that ran one chunk, total ms,
    tokens, the session)"""
    B, n = sig.shape
    rec = model.stream(B, precision="f32", beam_width=beam_width, max_frames=max_frames)
    if log:
        rec.encoded_log = []
    times, launches, ntok = [], [], 0
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for p0 in range(0, n, chunk):
        x = torch.from_numpy(sig[:, p0:p0 + chunk])
        l0, c0 = K.launch_count(), rec.chunks_run
        t0 = time.perf_counter()
        out = rec.accept(x)
        torch.cuda.synchronize()
        if rec.chunks_run == c0 + 1:
            times.append((time.perf_counter() - t0) * 1e3)
            launches.append(K.launch_count() - l0)
        ntok += int(out.tokens_length.sum())
    out = rec.finish()
    torch.cuda.synchronize()
    ntok += int(out.tokens_length.sum())
    return times, launches, (time.perf_counter() - t_all) * 1e3, ntok, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_beam_timing.json"))
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--widths", default="4,10")
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    OUT[0] = a.out
    dev = torch.device("cuda:0")
    cfg = configs.conformer_s(vocab_size=1000, chunk_size=16, history_size=64, convm_dw_norm="layer", sub_norm="layer", dropout=0.0)
    cfg.time_masking, cfg.freq_masking = {}, {}
    chunk = 640 * cfg.chunk_size  # samples of one chunk of audio
    max_frames = int(a.seconds * 25) + cfg.chunk_size
    RESULT.update(model="Conformer-S streaming (chunk 16, history 64, 16 blocks, V = 1000, random weights), f32 encoder", seconds=a.seconds,
                  chunk_audio_ms=cfg.chunk_size * 40.0, max_frames=max_frames, device=torch.cuda.get_device_name(0), runs=[])
    with limit(120):
        model = ConformerTransducer(cfg, dev, dtype=torch.bfloat16, seed=0)
        model.ps.p("joint/vocab/b")[0] += 0.7  # (random weights never emit the blank otherwise)
    rng = np.random.default_rng(0)
    for B in [int(v) for v in a.batches.split(",")]:
        sig = np.clip(rng.standard_normal((B, int(a.seconds * 16000))) * 0.1, -1, 1).astype(np.float32)
        for W in [int(v) for v in a.widths.split(",")]:
            r = dict(B=B, beam_width=W)
            with limit(240):  # warm-up utterances (workspaces, packed search weights, allocator)
                stream_once(model, sig, chunk, W, max_frames)
                stream_once(model, sig, chunk, 0, max_frames)
            beam_t, beam_l, greedy_t, greedy_l, totals = [], [], [], [], {"beam": [], "greedy": []}
            rec = None
            for _ in range(a.rounds):  # the two sessions alternate
                with limit(240):
                    t, l, total, ntok, rec = stream_once(model, sig, chunk, W, max_frames, log=True)
                beam_t += t
                beam_l += l
                totals["beam"].append(total)
                r["committed_tokens"] = ntok
                with limit(240):
                    t, l, total, ntok, _ = stream_once(model, sig, chunk, 0, max_frames)
                greedy_t += t
                greedy_l += l
                totals["greedy"].append(total)
                r["greedy_tokens"] = ntok
            r.update(chunks=len(beam_t), chunk_ms_median=statistics.median(beam_t), chunk_ms_worst=max(beam_t), chunk_ms_best=min(beam_t),
                     launches_per_chunk_median=statistics.median(beam_l), launches_per_chunk_max=max(beam_l),
                     greedy_chunk_ms_median=statistics.median(greedy_t), greedy_chunk_ms_worst=max(greedy_t),
                     greedy_launches_per_chunk_median=statistics.median(greedy_l), streamed_total_ms=min(totals["beam"]),
                     greedy_streamed_total_ms=min(totals["greedy"]))
            r["beam_over_greedy_chunk_median"] = r["chunk_ms_median"] / r["greedy_chunk_ms_median"]
            with limit(240):  # the offline search over the very frames the last beam session saw
                per = [torch.cat([e[b, :nv[b]] for e, nv in rec.encoded_log], 0) for b in range(B)]
                lens = [int(p.shape[0]) for p in per]
                enc = torch.zeros(B, max(lens), per[0].shape[1], dtype=per[0].dtype, device=dev)
                for b, p in enumerate(per):
                    enc[b, :lens[b]] = p
                model.recognize_beam_encoded(enc, lens, W, W)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                off = model.recognize_beam_encoded(enc, lens, W, W)
                torch.cuda.synchronize()
                r["offline_beam_encoded_ms"] = (time.perf_counter() - t0) * 1e3
                r["frames"] = max(lens)
                r["nbest_equals_offline_bitwise"] = all(torch.equal(x, y) for x, y in zip(rec.hypotheses(W), off[:3]))
            r["keeps_up_with_a_microphone"] = r["chunk_ms_worst"] < RESULT["chunk_audio_ms"]
            RESULT["runs"].append(r)
            print(json.dumps(r), flush=True)
            _write()
    _write()


if __name__ == "__main__":
    main()
