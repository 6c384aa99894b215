"""Token times and confidences of an n-best list: what the one-launch alignment costs next to the search and to the per-path baseline.
  python tools/nbest_detail_timing.py [--reps 7] [--out profiles/nbest_detail_timing.json]
Two shapes, seeded random logits (x 3) of 32 utterances x 250 frames: V = 1000 and V = 29, beam 10, 4 paths, the token array [32, 4, 250]
as the search returns it.  Three things, alternated call by call in one process so that they see the same clocks, HIP events around one
call after warm-up, [median, min, max] over `reps` rounds:
  nbest_align : ctc_nbest_align alone (tfasr_ctc_nbest_align: one lse / entropy pass per utterance, all 128 label rows in one walk);
  search      : ctc_beam_search_device alone;
  per_path    : the baseline the library offered before: 4 calls of ctc_align (tfasr_ctc_align) on the same logits, one per path, each
                with its own lse pass and its own copy of the path's token row (it gives no entropies).
The outputs of the two alignments are compared bit for bit; mean_tokens says how long the hypotheses are (the walk's time depends on
the frames, not on them: one thread per state of the padded width)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from tensorflowasr_amd import kernels as K

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("nbest_detail_timing: no GPU (timings are taken on the device only)")
dev = torch.device("cuda", 0)
B, T, W, P = 32, 250, 10, 4


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return [round(float(np.median(ms)), 3), round(float(min(ms)), 3), round(float(max(ms)), 3)]


doc = {"note": "[median, min, max] ms over rounds that alternate the three calls, HIP events around one call; 32 x 250 frames, seeded random "
               "logits x 3, beam 10, 4 paths", "shapes": []}
for V in (1000, 29):
    rng = np.random.default_rng(V)
    x = torch.from_numpy((rng.standard_normal((B, T, V)) * 3.0).astype(np.float32)).to(dev)
    ln = torch.full((B,), T, dtype=torch.int32, device=dev)
    tokens, lengths, score = [t.clone() for t in K.ctc_beam_search_device(x, ln, beam_width=W, top_paths=P)]
    U = min(T, K.ALIGN_CTC_MAX_U)
    calls = {
        "nbest_align": lambda: K.ctc_nbest_align(x, ln, tokens, lengths, blank=V - 1),
        "search": lambda: K.ctc_beam_search_device(x, ln, beam_width=W, top_paths=P),
        "per_path": lambda: [K.ctc_align(x, tokens[:, p, :U].contiguous(), lengths[:, p].contiguous(), ln, blank=V - 1) for p in range(P)],
    }
    for fn in calls.values():  # warm-up: workspaces, code objects
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(args.reps):
        for k, fn in calls.items():
            ms[k].append(once(fn))
    row = dict(V=V, beam=W, paths=P, label_width=U, mean_tokens=round(float(lengths.float().mean()), 1))
    for k in calls:
        row[k + "_ms"] = stats(ms[k])
    row["nbest_align_over_per_path"] = round(row["nbest_align_ms"][0] / row["per_path_ms"][0], 3)
    row["nbest_align_over_search"] = round(row["nbest_align_ms"][0] / row["search_ms"][0], 3)
    new = [t.clone() for t in K.ctc_nbest_align(x, ln, tokens, lengths, blank=V - 1)]
    same = True
    for p in range(P):
        old = K.ctc_align(x, tokens[:, p, :U].contiguous(), lengths[:, p].contiguous(), ln, blank=V - 1)
        same = same and all(bool(torch.equal(a, b)) for a, b in zip((new[0][:, p, :U], new[1][:, p, :U], new[2][:, p, :U], new[4][:, p]), old))
    row["outputs_bit_equal"] = same
    doc["shapes"].append(row)
    print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
