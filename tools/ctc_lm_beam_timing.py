"""CTC prefix beam search with n-gram LM shallow fusion: what the fusion costs, and that the plain search did not get slower.
  python tools/ctc_lm_beam_timing.py [--reps 9] [--rounds 5] [--parent-lib PATH] [--out profiles/ctc_lm_beam_timing.json]
Two shapes, seeded random logits (x 3) of 32 utterances x 250 frames: V = 1000 at beam 10 with an order-3 model, V = 29 at beam 32 with
an order-5 model (NGramLM.estimate over seeded Markov-chain sequences).  Per shape, HIP events around one call after warm-up, [median,
min, max] over `reps` calls: the fused device search (tfasr_ctc_beam_search_lm), the plain device search (tfasr_ctc_beam_search), the
fused host routine (logits copied to host memory + tfasr_ctc_beam_search_lm_host), the fused device search at zero weights (the
plain search's hypotheses, so the difference to the plain search is what the fusion's mechanics cost); whether device and host agree,
and how long the hypotheses are (the searches' time depends on them).
--parent-lib: a build of the parent commit's library (same ABI).  The plain search is then called straight through ctypes on both
libraries, alternating parent / here for `rounds` rounds in this one sitting; the record lists every round's median, the spread of
the parent's rounds, and whether this tree's median lies inside it.  The two libraries' outputs are compared bit for bit."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.lm import NGramLM

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("ctc_lm_beam_timing: no GPU (timings are taken on the device only)")
dev = torch.device("cuda", 0)
B, T = 32, 250
SHAPES = [dict(V=1000, W=10, order=3), dict(V=29, W=32, order=5)]
ALPHA, BETA = 0.5, 0.1


def markov_sequences(V, n, seed):
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


def timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return [round(float(np.median(ms)), 3), round(float(min(ms)), 3), round(float(max(ms)), 3)]


def bind(path):
    lib = ctypes.CDLL(path)
    for name in ("tfasr_ctc_beam_search", "tfasr_ctc_beam_search_workspace_size", "tfasr_abi_version"):
        res, at = _lib.SIGNATURES[name]
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, at
    return lib


def plain_call(lib, x, ln, W, ws, out):
    toks, n, lp = out
    st = lib.tfasr_ctc_beam_search(x.data_ptr(), ln.data_ptr(), B, T, x.shape[2], W, 1, 0, 0, toks.data_ptr(), n.data_ptr(), lp.data_ptr(),
                                   ws.data_ptr(), ws.numel(), K._stream())
    assert st == 0, st


doc = {"note": "[median, min, max] ms over repetitions, HIP events around one call; 32 x 250 frames, seeded random logits x 3",
       "alpha_beta": [ALPHA, BETA], "shapes": []}
for sh in SHAPES:
    V, W, order = sh["V"], sh["W"], sh["order"]
    rng = np.random.default_rng(V)
    x = torch.from_numpy((rng.standard_normal((B, T, V)) * 3.0).astype(np.float32)).to(dev)
    ln = torch.full((B,), T, dtype=torch.int32)
    ln_dev = ln.to(dev)
    lm = NGramLM.estimate(markov_sequences(V, 400, V), order, V, 0)
    tables = lm.tables(ALPHA, BETA)
    row = dict(sh, lm_nodes=tables.nodes, lm_table_slots=tables.table_size)
    row["fused_device_ms"] = timed(lambda: K.ctc_beam_search_lm(x, ln_dev, tables, beam_width=W, blank_index=0), args.reps)
    row["plain_device_ms"] = timed(lambda: K.ctc_beam_search_device(x, ln_dev, beam_width=W, blank_index=0), args.reps)
    zero = lm.tables(0.0, 0.0)  # the plain search's hypotheses, found the fused way: what the fusion's mechanics cost on equal work
    row["fused_zero_weights_device_ms"] = timed(lambda: K.ctc_beam_search_lm(x, ln_dev, zero, beam_width=W, blank_index=0), args.reps)
    row["fused_host_ms"] = timed(lambda: K.ctc_beam_search_lm_host(x, ln, tables, beam_width=W, blank_index=0), max(3, args.reps // 3), warmup=1)
    row["fused_over_plain"] = round(row["fused_device_ms"][0] / row["plain_device_ms"][0], 2)
    row["fused_zero_weights_over_plain"] = round(row["fused_zero_weights_device_ms"][0] / row["plain_device_ms"][0], 2)
    row["host_over_device_fused"] = round(row["fused_host_ms"][0] / row["fused_device_ms"][0], 1)
    d = [t.cpu() for t in K.ctc_beam_search_lm(x, ln_dev, tables, beam_width=W, blank_index=0)]
    h = K.ctc_beam_search_lm_host(x, ln, tables, beam_width=W, blank_index=0)
    row["device_equals_host"] = bool(torch.equal(d[0], h[0]) and torch.equal(d[1], h[1]) and torch.equal(d[4], h[4]))
    p = [t.cpu() for t in K.ctc_beam_search_device(x, ln_dev, beam_width=W, blank_index=0)]
    row["fusion_changes_utterances"] = int((d[0][:, 0] != p[0][:, 0]).any(dim=1).sum())
    row["mean_tokens_fused"], row["mean_tokens_plain"] = round(float(d[1][:, 0].float().mean()), 1), round(float(p[1][:, 0].float().mean()), 1)
    if args.parent_lib:
        libs = {"parent": bind(args.parent_lib), "here": bind(_lib.LIB_PATH)}
        assert libs["parent"].tfasr_abi_version() == libs["here"].tfasr_abi_version()
        nbytes = ctypes.c_size_t(0)
        assert libs["here"].tfasr_ctc_beam_search_workspace_size(B, T, V, W, ctypes.byref(nbytes)) == 0
        ws = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
        outs = {who: K._paths(B, 1, T, dev) for who in libs}
        rounds = {who: [] for who in libs}
        for _ in range(args.rounds):
            for who in ("parent", "here"):
                rounds[who].append(timed(lambda: plain_call(libs[who], x, ln_dev, W, ws, outs[who]), args.reps)[0])
        torch.cuda.synchronize()
        pm, hm = rounds["parent"], rounds["here"]
        row["plain_search_vs_parent"] = {
            "parent_round_medians_ms": pm, "here_round_medians_ms": hm,
            "parent_median_ms": round(float(np.median(pm)), 3), "here_median_ms": round(float(np.median(hm)), 3),
            "parent_spread_ms": [min(pm), max(pm)], "here_spread_ms": [min(hm), max(hm)], "here_over_parent": round(float(np.median(hm) / np.median(pm)), 4),
            "here_median_within_parent_spread": bool(np.median(hm) <= max(pm)),  # (below the parent's fastest round counts as within)
            "outputs_bit_equal": all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(outs["parent"], outs["here"])),
        }
    doc["shapes"].append(row)
    print(json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
