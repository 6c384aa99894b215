"""Streaming DeepSpeech2 timing on one MI355X -> profiles/deepspeech2_stream_timing.json.  A tool, not a test and not part of bench.py;
nothing is asserted and there is no threshold to meet.

The unidirectional config (uni.yml.j2: causal Conv2D, 5 forward LSTMs with RowConv1D, V = 29), 10 s of audio per stream, chunk_frames 32
(16 encoder frames a step), B = 1 and 32 streams, the bf16 model and its f32 twin.  Recorded:
  * one session step (`accept` of exactly one step's samples): wall time and device-event time,
  * a whole utterance streamed (one `accept` of everything, then `finish`) against offline `recognize` of the same audio,
  * (not timed) whether the streamed tokens are the offline ones, and at B = 1 whether the streamed encoder frames are bit for bit,
  * one layer's stateful recurrence (tfasr_lstm_infer_fwd_state, T = 16, the model's P) on the persistent launch against the same call
    under tfasr_lstm_set_persist(0) (the per-step kernels), the two ALTERNATED in one process so that clock drift hits both alike.
Method: warm-up, then the median of the repeats with min and max stated; clocks as the machine's governor leaves them (not pinned);
weights are random (time does not depend on them).

Usage: python tools/deepspeech2_stream_timing.py [--batch 32] [--seconds 10] [--repeats 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tensorflowasr_amd import configs  # noqa: E402
from tensorflowasr_amd import kernels as K  # noqa: E402
from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC  # noqa: E402
from tensorflowasr_amd.schemas import PredictInput  # noqa: E402


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def timed(fn, warmup, repeats):
    """-> (device-event stats, wall stats) of fn"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(a.elapsed_time(b))
    return stats(dev_ms), stats(wall_ms)


def recurrence(dev, B, T, P, warmup, repeats):
    """one layer's stateful recurrence in bf16, persistent launch and per-step kernels alternated"""
    g = torch.Generator().manual_seed(B)
    xg = (torch.randn(B, T, 4 * P, generator=g) * 0.7).to(torch.bfloat16).to(dev)
    rk = (torch.randn(1, P, 4 * P, generator=g) / np.sqrt(P)).to(torch.bfloat16).to(dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    s = [tuple(torch.zeros(B, P, device=dev) for _ in range(2)) for _ in range(2)]
    y = torch.empty(B, T, P, dtype=torch.bfloat16, device=dev)
    ms = {0: [], 1: []}
    prev = K.lstm_set_persist(1)
    try:
        for it in range(warmup + repeats):
            for mode in (1, 0):
                K.lstm_set_persist(mode)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                K.lstm_infer_fwd(xg, rk, lens, y=y, state=s[0], state_out=s[1])
                b.record()
                torch.cuda.synchronize()
                if it >= warmup:
                    ms[mode].append(a.elapsed_time(b))
    finally:
        K.lstm_set_persist(prev)
    return dict(B=B, T=T, P=P, persistent=stats(ms[1]), per_step=stats(ms[0]),
                per_step_over_persistent=statistics.median(ms[0]) / statistics.median(ms[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepspeech2_stream_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n = int(a.seconds * 16000)
    cfg = configs.deepspeech2(vocab_size=29, variant="uni")
    chunk = 32
    out = dict(device=torch.cuda.get_device_name(0), clocks="governor default, not pinned", config="deepspeech2 uni, V = 29",
               rnn_nlayers=int(cfg.rnn_nlayers), rnn_units=int(cfg.rnn_units), seconds=a.seconds, chunk_frames=chunk, warmup=a.warmup,
               repeats=a.repeats, method="median of repeats (min and max stated); device events and host wall clock", runs=[], recurrence=[])
    model = DeepSpeech2CTC(cfg, dev, dtype=torch.bfloat16, seed=0)
    for prec in ("bf16", "f32"):
        model.decode_precision = prec
        for B in (1, a.batch):
            sig = np.clip(rng.standard_normal((B, n)) * 0.1, -1, 1).astype(np.float32)
            x = PredictInput(torch.from_numpy(sig), torch.full((B,), n, dtype=torch.int32))
            rec = model.stream(B, chunk_frames=chunk, precision=prec)
            step = torch.from_numpy(sig[:, :chunk * cfg.frame_step].copy())
            rec.accept(step)  # fills the first frame's window; every later accept of one step's samples runs exactly one step
            step_dev, step_wall = timed(lambda: rec.accept(step), a.warmup, a.repeats)

            def streamed():
                r = model.stream(B, chunk_frames=chunk, precision=prec)
                r.accept(x.inputs)
                r.finish()

            # not timed: the streamed run is the offline run (tokens of every stream; at B = 1 also the encoder frames, bit for bit)
            r = model.stream(B, chunk_frames=chunk, precision=prec)
            r.encoded_log = []
            o1, o2 = r.accept(x.inputs), r.finish()
            got = [o1.tokens[b, :int(o1.tokens_length[b])].tolist() + o2.tokens[b, :int(o2.tokens_length[b])].tolist() for b in range(B)]
            want = [[t for t in row if t != model.blank] for row in model.recognize(x).tokens.cpu().tolist()]
            same_frames = None
            if B == 1:
                enc, elen = model.encode(x.inputs, x.inputs_length, precision=prec)
                frames = torch.cat([e[0, :nv[0]] for e, nv in r.encoded_log if nv[0]])
                same_frames = bool(frames.shape[0] == elen[0] and torch.equal(frames, enc[0, :elen[0]]))
            few = max(3, a.repeats // 4)
            utt_dev, utt_wall = timed(streamed, 1, few)
            off_dev, off_wall = timed(lambda: model.recognize(x), 1, few)
            run = dict(precision=prec, B=B, streamed_tokens_equal_offline=got == want, tokens=sum(len(t) for t in want),
                       streamed_frames_bit_equal_offline=same_frames, step_device=step_dev, step_wall=step_wall, steps_per_utterance=-(-(-(-n // cfg.frame_step)) // chunk),
                       streamed_utterance_wall=utt_wall, offline_recognize_wall=off_wall,
                       streamed_over_offline=utt_wall["median_ms"] / off_wall["median_ms"],
                       streamed_rtf=utt_wall["median_ms"] / 1e3 / (B * a.seconds), offline_rtf=off_wall["median_ms"] / 1e3 / (B * a.seconds))
            print(json.dumps(run), flush=True)
            out["runs"].append(run)
    for B in (1, a.batch):
        r = recurrence(dev, B, chunk // cfg.time_reduction_factor, int(cfg.rnn_units), a.warmup, a.repeats)
        print(json.dumps(r), flush=True)
        out["recurrence"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
