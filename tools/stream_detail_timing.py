"""What token times and confidences cost in a streaming session (Conformer-S streaming config, V = 1000, 10 s per stream, B = 1 and 32,
bf16 encoder; transducer and CTC head), and the one-launch CTC kernel against the two-launch plain one.
  python tools/stream_detail_timing.py [--reps 7] [--sitting FILE ...] [--out profiles/stream_detail_timing.json]
The method of tools/recognize_detail_timing.py: HIP events after warm-up, [median, min, max] over N repetitions, the two variants
alternated inside one loop so that both see the same clocks; spread = (max - min) / median of a row, the run-to-run noise a difference is
read against.  A session step = one 640 ms chunk: a whole 10 s utterance goes through accept() chunk by chunk and finish(), and the time
is divided by the chunks the session ran.
--plain-only [--label NAME]: time the plain session alone and print one JSON line; it uses nothing this change adds, so this same
file, started with a built checkout of the parent commit as its working directory (that checkout's package is then the one imported), times
the parent.
--sitting FILE ...: such lines, measured one after the other just before in the same sitting (parent, this tree, parent), are listed in
order in front of this run's own two plain timings (first alternated with the detail session, then once more alone at the end): the processes
of the two trees alternate, and the list shows the drift within the sitting that a parent / here difference is read against."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())

import numpy as np
import torch

from tensorflowasr_amd import _lib, configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.ctc_model import ConformerCTC

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sitting", nargs="*", default=[])
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--label", default="here")
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
SECONDS, V, BATCHES = 10.0, 1000, (1, 32)
OVER = dict(vocab_size=V, chunk_size=16, history_size=64, convm_dw_norm="layer", sub_norm="layer", dropout=0.0)


def stats(xs):
    return [round(float(np.median(xs)), 4), round(float(min(xs)), 4), round(float(max(xs)), 4)]


def spread(row):
    return round((row[2] - row[1]) / row[0], 4)


def timed(fns, warm=2):
    """the calls of `fns` alternated: warm-up, then `reps` rounds, each call between its own pair of events -> [median, min, max] ms each"""
    for _ in range(warm):
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
    return ms


def utterance(model, sig, detail=False):
    """one utterance per stream through a session, one chunk of audio per accept -> (chunks run, tokens)"""
    chunk = 640 * model.cfg.chunk_size
    rec = (model.stream_detailed if detail else model.stream)(sig.shape[0], precision="bf16")
    ntok = 0
    for p0 in range(0, sig.shape[1], chunk):
        ntok += int(rec.accept(torch.from_numpy(sig[:, p0:p0 + chunk])).tokens_length.sum())
    ntok += int(rec.finish().tokens_length.sum())
    return rec.chunks_run, ntok


def build(head):
    cfg = configs.conformer_s(**OVER) if head == "transducer" else configs.conformer_ctc_s(**OVER)
    cfg.time_masking, cfg.freq_masking = {}, {}
    model = (ConformerTransducer if head == "transducer" else ConformerCTC)(cfg, dev, dtype=torch.bfloat16, seed=0)
    if head == "transducer":
        model.ps.p("joint/vocab/b")[0] += 0.7  # (tools/stream_timing.py: random weights never emit the blank otherwise)
    return model


def sessions(model, plain_only=False):
    rng = np.random.default_rng(0)
    res = {}
    for B in BATCHES:
        sig = np.clip(rng.standard_normal((B, int(SECONDS * 16000))) * 0.1, -1, 1).astype(np.float32)
        chunks, ntok = utterance(model, sig)
        variants = [lambda: utterance(model, sig)] + ([] if plain_only else [lambda: utterance(model, sig, detail=True)])
        rows = [stats([m / chunks for m in ms]) for ms in timed(variants)]
        r = {"chunks": chunks, "tokens": ntok, "plain_step_ms": rows[0]}
        if not plain_only:
            r.update(detail_step_ms=rows[1], spread=max(spread(rows[0]), spread(rows[1])), detail_over_plain=round(rows[1][0] / rows[0][0], 4),
                     same_tokens=utterance(model, sig, detail=True)[1] == ntok)
            r["difference_inside_spread"] = abs(r["detail_over_plain"] - 1) <= r["spread"]
        res[f"B={B}"] = r
    return res


def kernel_alone(C=16, calls=50):
    """the one-launch detail kernel against the plain carried decoder's two launches and, for the same work without the carry, the offline
    detail decoder's two launches; one chunk of f32 logits, pre-allocated buffers, `calls` calls back to back between one pair of events
    -> us per call"""
    lib, p, st = _lib.load(), K._p, K._stream
    res = {}
    for B in BATCHES:
        g = torch.Generator().manual_seed(B)
        logits = (torch.randn(B, C, V, generator=g) * 2).to(dev)
        ll = torch.full((B,), C, dtype=torch.int32, device=dev)
        fin = torch.zeros(B, dtype=torch.int32, device=dev)
        state = K.CtcDetailState(B, dev)
        ib, fb, tl = torch.empty(3, B, C + 1, dtype=torch.int32, device=dev), torch.empty(2, B, C + 1, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        last, ws, tok = torch.full((B,), -1, dtype=torch.int32, device=dev), torch.empty(3 * B * C, dtype=torch.int32, device=dev), torch.empty(B, C, dtype=torch.int32, device=dev)
        ob, of, score = torch.empty(3, B, C, dtype=torch.int32, device=dev), torch.empty(2, B, C, device=dev), torch.empty(B, device=dev)

        def detail():
            for _ in range(calls):
                K.check(lib.tfasr_ctc_greedy_decode_carry_detail(p(logits), p(ll), p(fin), p(state.ints), p(state.floats), p(ib[0]), p(tl), p(ib[1]),
                                                                 p(ib[2]), p(fb[0]), p(fb[1]), B, C, V, 0, 0, st()), "carry_detail")

        def plain():
            for _ in range(calls):
                K.check(lib.tfasr_ctc_greedy_decode_carry(p(logits), p(ll), p(last), p(ws), p(tok), p(tl), B, C, V, 0, 0, st()), "carry")

        def offline():
            for _ in range(calls):
                K.check(lib.tfasr_ctc_greedy_decode_detail(p(logits), p(ll), p(ws), p(ob[0]), p(tl), p(ob[1]), p(ob[2]), p(of[0]), p(of[1]), p(score),
                                                           B, C, V, 0, 0, st()), "detail")

        rows = [stats([m * 1e3 / calls for m in ms]) for ms in timed([plain, detail, offline])]
        res[f"B={B}"] = {"carry_two_launches_us": rows[0], "carry_detail_one_launch_us": rows[1], "offline_detail_two_launches_us": rows[2],
                         "spread": max(spread(r) for r in rows), "detail_over_plain": round(rows[1][0] / rows[0][0], 4),
                         "detail_over_offline_detail": round(rows[1][0] / rows[2][0], 4)}
    return res


out = {}
models = {}
for head in ("transducer", "ctc"):
    models[head] = build(head)
    out[head] = sessions(models[head], args.plain_only)
if args.plain_only:
    print(json.dumps({"label": args.label, "results": out}))
    sys.exit(0)

doc = {"shape": f"Conformer-S streaming config (chunk 16, history 64), bf16 encoder, search and CTC decisions in f32, {SECONDS:.0f} s per stream, V = {V}",
       "note": "session rows: [median, min, max] ms per 640 ms step (utterance time / chunks), HIP events, stream() and stream_detailed() sessions alternated "
               "in one loop; kernel rows: us per call of one 16-frame chunk, 50 calls back to back; spread = (max - min) / median",
       "sessions": out, "ctc_kernel_alone": kernel_alone()}
if args.sitting:
    runs = []
    for path in args.sitting:
        with open(path) as f:
            runs.append(json.loads(f.read().strip().splitlines()[-1]))
    again = {head: sessions(m, plain_only=True) for head, m in models.items()}
    runs += [{"label": "here (alternated with detail)", "results": out}, {"label": "here (again, alone)", "results": again}]
    doc["sitting"] = {"order": [r["label"] for r in runs]}
    for head in out:
        for b in out[head]:
            rows = [r["results"][head][b]["plain_step_ms"] for r in runs]
            med = {who: [row[0] for r, row in zip(runs, rows) if r["label"].startswith(who)] for who in ("parent", "here")}
            doc["sitting"][f"{head} {b}"] = {
                "plain_step_ms": rows, "parent_medians": med["parent"], "here_medians": med["here"],
                "here_over_parent": round(float(np.mean(med["here"]) / np.mean(med["parent"])), 4),
                "drift": round((max(med["parent"] + med["here"]) - min(med["parent"] + med["here"])) / float(np.median(med["parent"] + med["here"])), 4),
                "ranges_overlap": min(med["here"]) <= max(med["parent"]) and min(med["parent"]) <= max(med["here"])}
print(json.dumps(doc, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
