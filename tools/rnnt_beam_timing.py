"""Transducer beam search at the bench's decode shape (Conformer-M, bf16 model, f32 search, 32 x 10 s, V = 1000).
  python tools/rnnt_beam_timing.py [--reps N] [--out FILE.json]
On ONE encoder output (model.encode, the f32 twin), timed with HIP events after warm-up, [median, min, max] over N repetitions: the greedy
search (recognize_encoded, the bench's decode) and the device beam search (recognize_beam_encoded) at W = 1, 4 and 10 (top_paths
min(4, W)).  Also: how many utterances the W = 1 search decodes exactly like the greedy search at one symbol per frame
(recognize_encoded per utterance, max_tokens_per_frame=1), and the tokens emitted per utterance.  Two runs: the random-init blank bias
(its rows emit a label on every frame), and the blank bias
raised until the greedy search at one symbol per frame emits <= 7.4 tokens per second of audio (blanks and labels mixed)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())

import numpy as np
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd.conformer import ConformerTransducer

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
model = ConformerTransducer(configs.conformer_m(), dev, dtype=torch.bfloat16, seed=0)
rng = np.random.default_rng(0)
B, secs = 32, 10.0
n = int(secs * 16000)
sig = torch.from_numpy(np.clip(rng.standard_normal((B, n)).astype(np.float32) * 0.1, -1, 1)).to(dev)
enc, elen = model.encode(sig, torch.full((B,), n, dtype=torch.int32))
b0 = float(model.ps.p("joint/vocab/b")[0].item())


def timed(fn):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return [round(float(np.median(ms)), 3), round(float(min(ms)), 3), round(float(max(ms)), 3)]


def set_bias(delta):
    model.ps.p("joint/vocab/b")[0] = b0 + delta
    model.ps.refresh_shadow()


def greedy_one_per_frame():
    out = []
    for b, nb in enumerate(elen):
        t = model.recognize_encoded(enc[b:b + 1, :nb].contiguous(), [nb], max_tokens_per_frame=1).tokens[0].cpu().numpy()
        out.append(t[t != model.blank].tolist())
    return out


def run(delta):
    set_bias(delta)
    res = {"blank_bias_delta": delta, "greedy_ms": timed(lambda: model.recognize_encoded(enc, elen))}
    for W in (1, 4, 10):
        res[f"beam{W}_ms"] = timed(lambda: model.recognize_beam_encoded(enc, elen, W, min(4, W)))
    ref = greedy_one_per_frame()
    toks, lens = model.recognize_beam_encoded(enc, elen, 1, 1)[:2]
    w1 = [toks[b, 0, :int(lens[b, 0])].tolist() for b in range(B)]
    res["w1_equals_greedy_one_per_frame"] = f"{sum(a == g for a, g in zip(w1, ref))} / {B}"
    res["tokens_per_utterance_greedy_one_per_frame"] = round(float(np.mean([len(g) for g in ref])), 2)
    for W in (4, 10):
        lens = model.recognize_beam_encoded(enc, elen, W, 1)[1]
        res[f"tokens_per_utterance_beam{W}"] = round(float(lens.float().mean()), 2)
    res["beam4_over_greedy"] = round(res["beam4_ms"][0] / res["greedy_ms"][0], 2)
    return res


runs = [run(0.0)]
# second run: the blank bias moved until paths mix blanks and labels.  At this random init the rows emit a label on EVERY frame (the
# first run), so the bias is raised (as bench.py's decode calibration does), to the first value at which the greedy search at one symbol
# per frame emits <= 3.7 tokens per second of audio x 2
delta = 0.0
for d in (1.0, 2.0, 4.0, 8.0, 16.0):
    set_bias(d)
    delta = d
    if np.mean([len(g) for g in greedy_one_per_frame()]) <= 2 * 3.7 * secs:
        break
runs.append(run(delta))
set_bias(0.0)
out = {"shape": f"conformer_m bf16 model (f32 search on the f32 master weights), {B} x {secs:.0f} s, T' = {enc.shape[1]}, "
                f"P = {model.cfg.rnn_units}, J = {model.cfg.joint_dim}, V = {model.cfg.vocab_size}",
       "runs": runs,
       "note": "[median, min, max] ms over repetitions, HIP events, same encoder output; greedy = recognize_encoded (the bench's batch "
               "search, <= 3 symbols per frame); beamW = recognize_beam_encoded(W, top_paths = min(4, W))"}
print(json.dumps(out, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
