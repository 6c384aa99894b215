"""What token times and confidences cost: recognize against recognize_detailed (Conformer-S, V = 1000, 32 x 10 s; transducer and CTC).
  python tools/recognize_detail_timing.py [--reps 7] [--parent-json FILE] [--out profiles/recognize_detail_timing.json]
Timed with HIP events after warm-up, [median, min, max] ms over N repetitions on ONE batch, the two calls alternated inside one loop
so that both see the same clocks.  `spread` is (max - min) / median of a row: the run-to-run noise the ratios are read against.
--plain-only: time recognize alone and print one JSON line; needs nothing this change adds, so this same file, started with a built
checkout of the parent commit as its working directory (that checkout's package is then the one imported), times the parent.
--parent-json FILE: that line, measured just before in the same sitting, is set beside this tree's numbers; recognize is timed here
twice (first alternated with recognize_detailed, then once more alone at the end) to show the drift within the sitting.  recognize
itself must not have changed: its here / parent ratios should sit inside the spread."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())

import numpy as np
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.ctc_model import ConformerCTC
from tensorflowasr_amd.schemas import PredictInput

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--parent-json", default=None)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
B, secs, V = 32, 10.0, 1000
n = int(secs * 16000)
rng = np.random.default_rng(0)
sig = torch.from_numpy(np.clip(rng.standard_normal((B, n)).astype(np.float32) * 0.1, -1, 1))
inputs = PredictInput(sig, torch.full((B,), n, dtype=torch.int32))


def stats(ms):
    return [round(float(np.median(ms)), 3), round(float(min(ms)), 3), round(float(max(ms)), 3)]


def spread(row):
    return round((row[2] - row[1]) / row[0], 4)


def timed(fns):
    """the calls of `fns` alternated: warm-up twice, then `reps` rounds, each call between its own pair of events"""
    for _ in range(2):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(args.reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [stats(m) for m in ms]


def measure(model):
    if args.plain_only:
        return {"recognize_ms": timed([lambda: model.recognize(inputs)])[0]}
    plain, detailed = timed([lambda: model.recognize(inputs), lambda: model.recognize_detailed(inputs)])
    res = {"recognize_ms": plain, "recognize_detailed_ms": detailed, "spread": max(spread(plain), spread(detailed)),
           "detailed_over_plain": round(detailed[0] / plain[0], 4)}
    a, b = model.recognize(inputs), model.recognize_detailed(inputs)
    res["same_tokens"] = bool(torch.equal(a.tokens, b.predict.tokens))
    res["tokens"] = int((b.frames >= 0).sum())
    return res


rnnt = ConformerTransducer(configs.conformer_s(vocab_size=V), dev, dtype=torch.bfloat16, seed=0)
out = {"transducer": measure(rnnt)}
iters = getattr(rnnt, "last_search_iterations", None)
if iters and not args.plain_only:
    r = out["transducer"]
    r["search_iterations"] = int(iters)
    r["extra_us_per_iteration"] = round((r["recognize_detailed_ms"][0] - r["recognize_ms"][0]) * 1e3 / iters, 3)
out["ctc"] = measure(ConformerCTC(configs.conformer_ctc_s(vocab_size=V), dev, dtype=torch.bfloat16, seed=0))
if args.plain_only:
    print(json.dumps(out))
    sys.exit(0)


doc = {"shape": f"conformer_s / conformer_ctc_s, bf16 model (search and CTC decisions in f32), {B} x {secs:.0f} s, V = {V}",
       "note": "[median, min, max] ms, HIP events, recognize and recognize_detailed alternated in one loop; spread = (max - min) / median",
       "results": out}
if args.parent_json:
    del rnnt
    torch.cuda.empty_cache()
    with open(args.parent_json) as f:
        after = json.loads(f.read().strip().splitlines()[-1])
    again = {k: timed([lambda m=m: m.recognize(inputs)])[0] for k, m in
             (("transducer", ConformerTransducer(configs.conformer_s(vocab_size=V), dev, dtype=torch.bfloat16, seed=0)),
              ("ctc", ConformerCTC(configs.conformer_ctc_s(vocab_size=V), dev, dtype=torch.bfloat16, seed=0)))}
    doc["parent"] = {k: {"recognize_ms": after[k]["recognize_ms"], "recognize_here_again_ms": again[k],
                         "here_over_parent": round(out[k]["recognize_ms"][0] / after[k]["recognize_ms"][0], 4),
                         "here_again_over_parent": round(again[k][0] / after[k]["recognize_ms"][0], 4)} for k in ("transducer", "ctc")}
print(json.dumps(doc, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
