"""Streaming Transformer timing on one MI355X -> profiles/transformer_stream_timing.json.  A tool, not a test and not part of bench.py;
nothing is asserted.  base-streaming config (examples/models/ctc/transformer/base-streaming.yml.j2: d 512, 4 heads of 128, 6 blocks,
chunk 16, history 64), V = 29, 10 s of audio per stream, B = 1 and 32 streams, bf16 and f32.

tools/transformer_timing.py's method: every version is measured against its baseline in the same call, ALTERNATED (a, b, a, b, ...),
medians of 7 repeats with the spread (max - min) / median next to each median, device events around the region (each timed region runs the
call `inner` times, the figure is per call), clocks as the machine's governor leaves them (not pinned); weights and inputs are random.
  * one layer's attention step on a fused projection output [B C, 3 H dh] with full rings (seen = 200): tfasr_stream_attn_plain_fwd (the
    attention and the ring append, one launch) against what the library could do before it - tfasr_stream_attn_fwd fed an all-zero
    position table [hist + 2C - 1, H dh] and zero biases, then tfasr_stream_kv_append.  The table and the biases are allocated and cleared
    once per session, outside the timed region: only their reads count against the baseline.
  * the whole encode_chunk step (every stream with a full chunk) and its kernel launches,
  * a streamed 10 s utterance per stream (accept the whole audio, finish) against offline `recognize` of the same audio, with the RTF
    (wall time / audio time) of both.
"slower" below means by more than the larger of the two spreads.

Usage: python tools/transformer_stream_timing.py [--batches 1 32] [--seconds 10] [--repeats 7]"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tensorflowasr_amd import configs  # noqa: E402
from tensorflowasr_amd import kernels as K  # noqa: E402
from tensorflowasr_amd.schemas import PredictInput  # noqa: E402
from tensorflowasr_amd.transformer import TransformerCTC  # noqa: E402
from transformer_timing import alternated  # noqa: E402


def compare(r, new, base):
    a, b = r[new], r[base]
    noise = max(a["spread"] * a["median_ms"], b["spread"] * b["median_ms"])
    r["baseline_over_new"] = b["median_ms"] / a["median_ms"]
    r["new_is_slower_by_more_than_the_spread"] = bool(a["median_ms"] - b["median_ms"] > noise)
    r["new_is_faster_by_more_than_the_spread"] = bool(b["median_ms"] - a["median_ms"] > noise)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer_stream_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    cfg0 = configs.transformer(vocab_size=29, streaming=True)
    C, hist, H, dh = cfg0.chunk_size, cfg0.history_size, cfg0.num_heads, cfg0.head_size
    HD, scale = H * dh, 1.0 / math.sqrt(dh)
    out = dict(device=torch.cuda.get_device_name(0), clocks="governor default, not pinned", warmup=a.warmup, repeats=a.repeats,
               config=f"base-streaming: chunk {C}, history {hist}, {H} heads of {dh}, d {cfg0.dmodel}, {cfg0.num_blocks} blocks, V 29",
               seconds_per_stream=a.seconds,
               method="versions alternated in one call, median of repeats, spread = (max - min) / median, device events",
               baseline="tfasr_stream_attn_fwd on an all-zero position table and zero biases + tfasr_stream_kv_append (two launches); the "
                        "table's allocation and clearing are per session and outside the timed region", runs={})
    n = int(a.seconds * 16000)
    for B in a.batches:
        sig = torch.from_numpy(np.clip(rng.standard_normal((B, n)) * 0.1, -1, 1).astype(np.float32))
        x = PredictInput(sig, torch.full((B,), n, dtype=torch.int32))
        g = torch.Generator().manual_seed(0)
        qkv32 = torch.randn(B * C, 3 * HD, generator=g).to(dev)
        seen, nvalid = torch.full((B,), 200, dtype=torch.int32, device=dev), torch.full((B,), C, dtype=torch.int32, device=dev)
        for dtype, prec in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
            tag, rec = f"B{B}_{prec}", {}
            qkv = qkv32.to(dtype)
            rings = [(torch.randn(B, hist, HD, generator=g) * 0.5).to(dtype).to(dev) for _ in range(4)]
            zero_u, zero_pos = torch.zeros(HD, device=dev), torch.zeros(hist + 2 * C - 1, HD, dtype=dtype, device=dev)  # once per session

            def new():
                K.stream_attn_plain_fwd(qkv, rings[0], rings[1], seen, nvalid, B, C, H, dh, hist, scale)

            def base():
                K.stream_attn_fwd(qkv, zero_u, zero_u, zero_pos, rings[2], rings[3], seen, nvalid, B, C, H, dh, hist, scale)
                K.stream_kv_append(qkv, rings[2], rings[3], seen, nvalid, B, C, H, dh, hist)

            rec["attention_step"] = compare(alternated({"plain_fused_append": new, "zero_table_baseline": base}, a.warmup, a.repeats, 50),
                                            "plain_fused_append", "zero_table_baseline")
            print(json.dumps({tag: {"attention_step": rec["attention_step"]}}), flush=True)
            model = TransformerCTC(configs.transformer(vocab_size=29, streaming=True), dev, dtype=dtype, seed=0)
            model.decode_precision = prec
            state = model.stream_state(B, precision=prec)
            feats = torch.randn(B, 4 * C, cfg0.num_feature_bins, generator=g).to(dtype).to(dev)
            take = [4 * C] * B

            def step():
                if state.host_seen[0] > 2000:  # (the position of a stream does not change the work of a step; keep the table small)
                    state.reset()
                model.encode_chunk(state, feats, take)

            for _ in range(6):  # fill the rings: the timed steps see full history
                step()
            before = K.launch_count()
            step()
            rec["encode_chunk_launches"] = K.launch_count() - before
            rec["encode_chunk"] = alternated({"step": step}, a.warmup, a.repeats, 10)["step"]

            def streamed():
                s = model.stream(B, precision=prec)
                s.accept(sig)
                s.finish()

            r = alternated({"streamed": streamed, "offline_recognize": lambda: model.recognize(x, precision=prec)}, 1, max(3, a.repeats // 2))
            s = model.stream(B, precision=prec)
            s.accept(sig)
            s.finish()
            r.update(chunks=s.chunks_run, streamed_rtf=r["streamed"]["median_ms"] / 1e3 / (B * a.seconds),
                     offline_rtf=r["offline_recognize"]["median_ms"] / 1e3 / (B * a.seconds),
                     streamed_over_offline=r["streamed"]["median_ms"] / r["offline_recognize"]["median_ms"])
            rec["utterance"] = r
            print(json.dumps({tag: {k: rec[k] for k in ("encode_chunk_launches", "encode_chunk", "utterance")}}), flush=True)
            out["runs"][tag] = rec
            del model, state
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
