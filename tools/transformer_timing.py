"""Transformer CTC timing on one MI355X -> profiles/transformer_timing.json.  A tool, not a test and not part of bench.py; nothing is
asserted.  Base config (examples/models/ctc/transformer/base.yml.j2: d 512, 4 heads of 128, 6 blocks), V = 29, batches of 32 x 10 s
(T' = 250) and 32 x 35 s (T' = 875), every utterance full length.

Every version is measured against its baseline in the same call, ALTERNATED (a, b, a, b, ...), medians of the repeats, and the spread
(max - min) / median of the repeated identical runs recorded next to each median; device events around the region (each timed region
runs the call `inner` times, the figure is per call), clocks as the machine's governor leaves them (not pinned); weights and inputs are
random (time does not depend on them):
  * one attention layer on a fused projection output [B T', 3 H dh], bf16 and f32: tfasr_attn_plain_fwd (csrc/attn_plain.hip) against what
    the library could do before it - batched tfasr_gemm for scale Q K^T, tfasr_relattn_softmax_fwd_streaming fed a ZERO position tensor
    [B, H, T', 2T'], batched tfasr_gemm for P V (transformer.unfused_attention).  The zero tensor is allocated and cleared inside the timed
    region and its read by the softmax counts against the baseline: the baseline cannot run without it.
  * the whole encoder on both routes, and `recognize` (the model's own choice of route: fused in bf16, unfused in f32) with its RTF
    (wall time / audio time), bf16 and the f32 twin,
  * one run of the chunked config (base-streaming.yml.j2: chunk 16, history 64) at 32 x 10 s.
"slower" below means by more than the larger of the two spreads.

Usage: python tools/transformer_timing.py [--batch 32] [--seconds 10 35] [--repeats 7]"""
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
from tensorflowasr_amd import kernels as K  # noqa: E402
from tensorflowasr_amd.schemas import PredictInput  # noqa: E402
from tensorflowasr_amd.transformer import TransformerCTC, unfused_attention  # noqa: E402


def once(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def alternated(fns, warmup, repeats, inner=1):
    """{name: fn} -> {name: dict(median_ms, spread, all_ms)}, the versions taking turns"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(once(fn, inner))
    return {k: dict(median_ms=statistics.median(v), spread=(max(v) - min(v)) / statistics.median(v), all_ms=v) for k, v in ms.items()}


def compare(r, new, base):
    a, b = r[new], r[base]
    noise = max(a["spread"] * a["median_ms"], b["spread"] * b["median_ms"])
    r["baseline_over_fused"] = b["median_ms"] / a["median_ms"]
    r["fused_is_slower_by_more_than_the_spread"] = bool(a["median_ms"] - b["median_ms"] > noise)
    r["fused_is_faster_by_more_than_the_spread"] = bool(b["median_ms"] - a["median_ms"] > noise)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 35.0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    out = dict(device=torch.cuda.get_device_name(0), clocks="governor default, not pinned", batch=a.batch, warmup=a.warmup, repeats=a.repeats,
               method="versions alternated in one call, median of repeats, spread = (max - min) / median, device events",
               baseline="batched tfasr_gemm (scale Q K^T) + tfasr_relattn_softmax_fwd_streaming on a zero position tensor [B, H, T', 2T'] + "
                        "batched tfasr_gemm (P V); the zero tensor's allocation, clearing and read are inside the timed region and count "
                        "against the baseline", shapes={})
    cfg0 = configs.transformer(vocab_size=29)
    H, dh = cfg0.num_heads, cfg0.head_size
    scale = 1.0 / float(np.sqrt(dh))
    for seconds in a.seconds:
        n = int(seconds * 16000)
        T = cfg0.encoder_length(-(-n // cfg0.frame_step))
        B = a.batch
        tag = f"{B}x{seconds:g}s"
        rec = dict(T_encoder=T, attention_flop=4 * B * H * T * T * dh)
        sig = torch.from_numpy(np.clip(rng.standard_normal((B, n)) * 0.1, -1, 1).astype(np.float32))
        x = PredictInput(sig, torch.full((B,), n, dtype=torch.int32))
        lens = torch.full((B,), T, dtype=torch.int32, device=dev)
        g = torch.Generator().manual_seed(0)
        qkv32 = torch.randn(B * T, 3 * H * dh, generator=g).to(dev)
        for dtype, prec in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
            qkv = qkv32.to(dtype)
            inner = 10 if dtype == torch.bfloat16 else 2
            r = alternated({"fused": lambda: K.attn_plain_fwd(qkv, lens, B, H, T, dh, scale),
                            "unfused_baseline": lambda: unfused_attention(qkv, lens, B, H, T, dh, scale)}, a.warmup, a.repeats, inner)
            compare(r, "fused", "unfused_baseline")
            r["fused_tflops"] = rec["attention_flop"] / (r["fused"]["median_ms"] / 1e3) / 1e12
            rec[f"attention_layer_{prec}"] = r
            print(json.dumps({tag: {f"attention_layer_{prec}": r}}), flush=True)
            model = TransformerCTC(configs.transformer(vocab_size=29), dev, dtype=dtype, seed=0)
            model.decode_precision = prec
            feats, flen = model.frontend(sig.to(dev), [n] * B)

            def encoder(route):
                def run():
                    model.attention_route = route
                    model.encoder_fwd(feats, flen, False, None)
                    model.attention_route = "auto"
                return run

            r = alternated({"fused": encoder("fused"), "unfused_baseline": encoder("unfused")}, 1, max(3, a.repeats // 2))
            compare(r, "fused", "unfused_baseline")
            rec[f"encoder_{prec}"] = r
            rr = alternated({"recognize": lambda: model.recognize(x)}, 1, max(3, a.repeats // 2))
            rr["recognize_rtf"] = rr["recognize"]["median_ms"] / 1e3 / (B * seconds)
            rr["attention_route"] = "fused" if dtype != torch.float32 else "unfused"
            rec[f"recognize_{prec}"] = rr
            print(json.dumps({tag: {f"encoder_{prec}": r, f"recognize_{prec}": rr}}), flush=True)
            del model
            torch.cuda.empty_cache()
        out["shapes"][tag] = rec
    # ---- the chunked config, once
    seconds = a.seconds[0]
    n = int(seconds * 16000)
    sig = torch.from_numpy(np.clip(rng.standard_normal((a.batch, n)) * 0.1, -1, 1).astype(np.float32))
    x = PredictInput(sig, torch.full((a.batch,), n, dtype=torch.int32))
    model = TransformerCTC(configs.transformer(vocab_size=29, streaming=True), dev, dtype=torch.bfloat16, seed=0)
    model.decode_precision = "bf16"
    feats, flen = model.frontend(sig.to(dev), [n] * a.batch)
    r = alternated({"encoder": lambda: model.encoder_fwd(feats, flen, False, None), "recognize": lambda: model.recognize(x)}, 1,
                   max(3, a.repeats // 2))
    r["recognize_rtf"] = r["recognize"]["median_ms"] / 1e3 / (a.batch * seconds)
    out["chunked_bf16"] = dict(shape=f"{a.batch}x{seconds:g}s", chunk_size=16, history_size=64, **r)
    print(json.dumps({"chunked_bf16": out["chunked_bf16"]}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
