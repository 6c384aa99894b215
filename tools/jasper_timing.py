"""Jasper CTC timing on one MI355X -> profiles/jasper_timing.json.  A tool, not a test and not part of bench.py; nothing is asserted.

Records, for the base (5 x 3) and 10x5 layouts in f32 and bf16, a batch of 32 x 10 s:
  * offline `recognize` and `recognize_beam(device_search=True)` as RTF (wall time / audio time),
  * the encoder's share of `recognize`, its achieved FLOP/s next to the formula 2 * sum K * Cin * Cout per encoder frame,
  * per-step latency of a streaming session at B = 1 and B = 32 (chunk_frames 32),
  * the baseline the Conv1D kernel replaces: the same layers as K accumulating tfasr_gemm calls per layer on shifted row views of the
    left-padded activations (f32 accumulator, no BatchNorm / residual / ReLU epilogue, which favours the baseline), same machine,
    same run, and the ratio baseline / kernel for the encoder's convolutions.
Method: warm-up, then the median of the repeats, device events around the region, clocks as the machine's governor leaves them (not
pinned); weights are random (time does not depend on them).

Usage: python tools/jasper_timing.py [--batch 32] [--seconds 10] [--repeats 5] [--layouts base,10x5]"""
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
from tensorflowasr_amd.jasper import JasperCTC  # noqa: E402
from tensorflowasr_amd.schemas import PredictInput  # noqa: E402


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def flops_per_frame(model):
    """2 * sum K * Cin * Cout over every Conv1D of the encoder, per ENCODER frame (the first block strides: it runs once per frame too)"""
    n = 0
    for m in model.layers:
        n += 2 * m["K"] * m["cin"] * m["cout"]
        n += sum(2 * rcin * m["cout"] for _, rcin, _ in m["residuals"] or [])
    return n


def gemm_baseline(model, feats):
    """every layer's convolution as K accumulating GEMMs on shifted row views (main convolutions and residual branches)"""
    B = feats.shape[0]
    x, residuals, starts = feats, [], model._block_starts()

    def conv(x, w, Kk, stride, dil):
        Bx, T, Cin = x.shape
        Cout, pad = w.shape[2], (Kk - 1) * dil
        pad += pad % 2
        xp = torch.zeros(Bx, pad + T, Cin, dtype=x.dtype, device=x.device)
        xp[:, pad:] = x
        lead = pad - (Kk - 1) * dil
        rows = (Bx * (pad + T) - pad) // stride
        flat = xp.view(-1)
        y = torch.empty(Bx * (pad + T) // stride, Cout, dtype=torch.float32, device=x.device)
        for k in range(Kk):
            K.gemm(flat[(lead + k * dil) * Cin:], w[k], y, rows, Cout, Cin, stride * Cin, Cout, Cout, accumulate=k > 0)
        return y.view(Bx, (pad + T) // stride, Cout)[:, :-(-T // stride)]

    for li, m in enumerate(model.layers):
        if li in starts:
            residuals.append(x)
        for rname, rcin, src in m["residuals"] or []:
            conv(residuals[src], model.ps.w(rname + "/pointwise_conv1d/w"), 1, 1, 1)
        y = conv(x, model.ps.w(m["name"] + "/conv1d/w"), m["K"], m["stride"], m["dilation"])
        x = y.to(x.dtype)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layouts", default="base,10x5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jasper_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n = int(a.seconds * 16000)
    sig = torch.from_numpy(np.clip(rng.standard_normal((a.batch, n)) * 0.1, -1, 1).astype(np.float32))
    x = PredictInput(sig, torch.full((a.batch,), n, dtype=torch.int32))
    audio_s = a.batch * a.seconds
    out = dict(device=torch.cuda.get_device_name(0), clocks="governor default, not pinned", batch=a.batch, seconds=a.seconds,
               warmup=a.warmup, repeats=a.repeats, method="median of repeats, device events", runs=[])
    for layout in a.layouts.split(","):
        for dtype, prec in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            model = JasperCTC(configs.jasper(vocab_size=1000, layout=layout), dev, dtype=dtype, seed=0)
            model.decode_precision = prec
            feats, flen = model.frontend(sig.to(dev), [n] * a.batch)
            torch.cuda.synchronize()
            t_rec, _ = timed(lambda: model.recognize(x), a.warmup, a.repeats)
            t_beam, _ = timed(lambda: model.recognize_beam(x, beam_width=10, device_search=True), a.warmup, a.repeats)
            t_enc, enc_all = timed(lambda: model.encoder_fwd(feats, flen, False, None), a.warmup, a.repeats)
            t_base, _ = timed(lambda: gemm_baseline(model, feats), a.warmup, a.repeats)
            frames = a.batch * model.cfg.encoder_length(feats.shape[1])
            fl = flops_per_frame(model) * frames
            run = dict(layout=layout, precision=prec, recognize_ms=t_rec, recognize_rtf=t_rec / 1e3 / audio_s, beam_ms=t_beam,
                       beam_rtf=t_beam / 1e3 / audio_s, encoder_ms=t_enc, encoder_ms_all=enc_all, encoder_share_of_recognize=t_enc / t_rec,
                       flop_per_encoder_frame=flops_per_frame(model), encoder_flop=fl, encoder_tflops=fl / (t_enc / 1e3) / 1e12,
                       gemm_per_tap_baseline_ms=t_base, baseline_over_kernel=t_base / t_enc, stream_step_ms={})
            for B in (1, a.batch):
                rec = model.stream(B, chunk_frames=32, precision=prec)
                step = torch.from_numpy(np.clip(rng.standard_normal((B, 32 * 160)) * 0.1, -1, 1).astype(np.float32))
                rec.accept(step)  # fills the first frame's window; every later accept of 5120 samples runs exactly one step
                t_step, _ = timed(lambda: rec.accept(step), a.warmup, min(a.repeats * 4, 20))
                run["stream_step_ms"][str(B)] = t_step
            print(json.dumps(run), flush=True)
            out["runs"].append(run)
            del model
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
