"""RNN-Transducer timing on one MI355X -> profiles/rnnt_timing.json.  A tool, not a test and not part of bench.py; nothing is asserted and
there is no threshold to meet.

The small config (examples/models/transducer/rnnt/small.yml.j2: 4 x (LSTM 1024 -> LayerNorm -> Dense 320), `post` reductions 3 and 2),
V = 1000, 32 utterances of 10 s (1000 feature frames -> 334 -> 167 encoder frames), the bf16 model and its f32 twin.  Every row compares
the block tail in one launch (tfasr_rnnt_block_tail_fwd, "fused") with the two-launch route (tfasr_layernorm_fwd + tfasr_gemm + the zero
fill, "unfused"), the two ALTERNATED in one process so that clock drift hits both alike:
  * the tail alone on layer 0's rows (32 x 1000, the un-reduced frame rate) and layer 3's (32 x 167),
  * block 0 (input projection, recurrence, tail) and the whole encoder,
  * `recognize` of the batch,
  * one 32-frame step of a streaming session's encoder (rnnt_encode_chunk) at 1 and 32 streams.
Method: warm-up, then the median of 7 repeats with min and max stated, device-event time around work that ends in a synchronise (a
repeat of the tail alone is 20 calls); clocks as the machine's governor leaves them (not pinned); weights are random (time does not depend
on them).

Usage: python tools/rnnt_timing.py [--batch 32] [--seconds 10] [--repeats 7] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tensorflowasr_amd import configs  # noqa: E402
from tensorflowasr_amd.rnnt import RnnTransducer  # noqa: E402
from tensorflowasr_amd.schemas import PredictInput  # noqa: E402


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def alternate(fns, warmup, repeats, inner=1):
    """{name: device-event stats of one call} of the callables, run in turn within every repeat"""
    ms = {k: [] for k in fns}
    for it in range(warmup + repeats):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if it >= warmup:
                ms[name].append(a.elapsed_time(b) / inner)
    out = {k: stats(v) for k, v in ms.items()}
    if "fused" in out and "unfused" in out:
        out["unfused_over_fused"] = out["unfused"]["median_ms"] / out["fused"]["median_ms"]
    return out


def routed(models, route, fn):
    def run():
        for m in models:
            m.tail_route = route
        try:
            return fn()
        finally:
            for m in models:
                m.tail_route = "auto"
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_timing.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnnt_timing needs an MI355X: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    cfg = configs.rnnt(vocab_size=1000)
    m16 = RnnTransducer(cfg, dev, dtype=torch.bfloat16, seed=1)
    m32 = m16.inference_twin()
    both = (m16, m32)
    B, n = a.batch, int(a.seconds * cfg.sample_rate)
    T0 = -(-n // cfg.frame_step)
    g = torch.Generator().manual_seed(0)
    sig = (torch.randn(B, n, generator=g) * 0.1).clamp_(-1, 1)
    x = PredictInput(sig, torch.full((B,), n, dtype=torch.int32), m16.get_initial_tokens(B), None, m16.get_initial_decoder_states(B))
    res = dict(config="small.yml.j2, V = 1000", batch=B, seconds=a.seconds, feature_frames=T0, encoder_frames=cfg.encoder_length(T0),
               repeats=a.repeats, device=torch.cuda.get_device_name(0), method="device events, fused / unfused alternated, median of repeats")
    for tag, m in (("bf16", m16), ("f32", m32)):
        r = res[tag] = {}
        mods = m.modules
        # the tail alone
        for layer, T in ((0, T0), (3, cfg.encoder_length(T0))):
            mod = mods[layer]
            y = (torch.randn(B, T, mod["P"], generator=g) * 0.5).to(m.dtype).to(dev)
            lens = torch.full((B,), T, dtype=torch.int32, device=dev)
            f = mod["factor"]
            Tpad = -(-T // f) * f
            fns = {k: routed(both, k, lambda: m.tail_fwd(y, mod, lens, Tpad, f)) for k in ("fused", "unfused")}
            out = {k: fn()[0].float() for k, fn in fns.items()}
            row = alternate(fns, a.warmup, a.repeats, inner=20)
            row.update(rows=B * T, P=mod["P"], N=mod["dout"], max_abs_difference=float((out["fused"] - out["unfused"]).abs().max()),
                       bytes_fused=B * T * (mod["P"] + mod["dout"]) * y.element_size(),
                       bytes_unfused=B * T * (3 * mod["P"] + mod["dout"]) * y.element_size())
            r[f"tail_layer{layer}"] = row
        # block 0 and the whole encoder on the model's own features
        feats, flen = m.frontend(sig.to(dev), [n] * B)
        lens0 = torch.full((B,), T0, dtype=torch.int32, device=dev)

        def block0():
            y = m.lstm_fwd(feats, mods[0], lens0)
            return m.tail_fwd(y, mods[0], lens0, -(-T0 // 3) * 3, 3)

        r["block0"] = alternate({k: routed(both, k, block0) for k in ("fused", "unfused")}, 1, a.repeats)
        r["encoder"] = alternate({k: routed(both, k, lambda: m.encoder_fwd(feats, flen, False, None)) for k in ("fused", "unfused")}, 1, a.repeats)
        m16.decode_precision = tag
        r["recognize"] = alternate({k: routed(both, k, lambda: m16.recognize(x)) for k in ("fused", "unfused")}, 1, a.repeats)
        # one 32-frame step of a session's encoder
        for streams in (1, B):
            chunk = feats[:streams, :32].contiguous()
            fns = {}
            for k in ("fused", "unfused"):
                st = routed(both, k, lambda: m.stream_state(streams, precision=tag))()
                fns[k] = routed(both, k, lambda st=st: m.encode_chunk(st, chunk, [32] * streams))
            r[f"stream_step_B{streams}"] = alternate(fns, a.warmup, a.repeats, inner=5)
    m16.decode_precision = "f32"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    for tag in ("bf16", "f32"):
        for k, v in res[tag].items():
            print(f"{tag:5s} {k:18s} fused {v['fused']['median_ms']:9.3f} ms   unfused {v['unfused']['median_ms']:9.3f} ms   x{v['unfused_over_fused']:.2f}")


if __name__ == "__main__":
    main()
