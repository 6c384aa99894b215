"""DeepSpeech2 CTC timing on one MI355X -> profiles/deepspeech2_timing.json.  A tool, not a test and not part of bench.py; nothing is
asserted.  Base config (base.yml.j2), V = 29, a batch of 32 x 10 s.

Every line is measured against its own baseline built from entry points that existed before the DeepSpeech2 kernels, both versions in
the same call, ALTERNATED (a, b, a, b, ...), medians of the repeats, and the spread (max - min) / median of the repeated identical runs
recorded next to each median; device events around the region, clocks as the machine's governor leaves them (not pinned); weights
and inputs are random (time does not depend on them):
  * conv module, bf16 and f32: the two tfasr_conv2d_fwd launches against the same two layers as F' calls of tfasr_conv1d_fwd each over
    pre-padded, materialised [B, T, kw * Cin] frequency windows (made outside the timed region, which favours the baseline; kw * Cin is
    rounded up to a multiple of 16 with zero taps; the time padding is the Conv1D's causal one, the work is the same),
  * one BiLSTM layer, B = 32, T' = 500, P = 512, bf16: ONE tfasr_lstm_infer_fwd launch over both directions against two sequential
    tfasr_lstm_persist_fwd calls on the same projections (the second on time-flipped input), and the per-step route,
  * whole `recognize` as RTF (wall time / audio time), f32 twin and bf16, and the encoder's parts.

Usage: python tools/deepspeech2_timing.py [--batch 32] [--seconds 10] [--repeats 7]"""
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
from tensorflowasr_amd.deepspeech2 import DeepSpeech2CTC  # noqa: E402
from tensorflowasr_amd.schemas import PredictInput  # noqa: E402


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternated(fns, warmup, repeats):
    """{name: fn} -> {name: dict(median_ms, spread, all_ms)}, the versions taking turns"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(once(fn))
    return {k: dict(median_ms=statistics.median(v), spread=(max(v) - min(v)) / statistics.median(v), all_ms=v) for k, v in ms.items()}


def conv1d_baseline(model, feats):
    """per conv block: (windows [F'] of [B, T, S16], Conv1D kernel in the compute type's layout, shape, time stride)"""
    dev, dtype = feats.device, feats.dtype
    x = feats.view(*feats.shape, 1)
    plan = []
    for m in model.modules["convs"]:
        B, T, F, Cin = x.shape
        pf, Fo = K.conv_pad_out(F, m["kw"], m["sf"], model.cfg.conv_padding)
        S = m["kw"] * Cin
        S16 = -(-S // 16) * 16
        xp = torch.zeros(B, T, (Fo - 1) * m["sf"] + m["kw"] + pf, Cin, dtype=dtype, device=dev)
        xp[:, :, pf:pf + F] = x
        wins = []
        for f in range(Fo):
            w = torch.zeros(B, T, S16, dtype=dtype, device=dev)
            w[:, :, :S] = xp[:, :, f * m["sf"]:f * m["sf"] + m["kw"]].reshape(B, T, S)
            wins.append(w)
        w1 = torch.zeros(m["kh"], S16, m["cout"], dtype=torch.float32, device=dev)
        w1[:, :S] = model.ps.p(m["name"] + "/conv2d/w").reshape(m["kh"], S, m["cout"])
        if dtype != torch.float32:
            w1 = K.conv1d_pack_weight(w1)
        plan.append((wins, w1, (m["kh"], S16, m["cout"]), m["st"]))
        wc, bias, scale, shift = model._conv_consts(m["name"])
        x = K.conv2d_fwd(x, wc, (m["kh"], m["kw"], m["cin"], m["cout"]), bias=bias, scale=scale, shift=shift, relu=True,
                         strides=(m["st"], m["sf"]), padding=model.cfg.conv_padding)

    def run():
        for wins, w1, shape, st in plan:
            for w in wins:
                K.conv1d_fwd(w, w1, shape, relu=True, stride=st)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deepspeech2_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n = int(a.seconds * 16000)
    sig = torch.from_numpy(np.clip(rng.standard_normal((a.batch, n)) * 0.1, -1, 1).astype(np.float32))
    x = PredictInput(sig, torch.full((a.batch,), n, dtype=torch.int32))
    audio_s = a.batch * a.seconds
    out = dict(device=torch.cuda.get_device_name(0), clocks="governor default, not pinned", batch=a.batch, seconds=a.seconds, warmup=a.warmup,
               repeats=a.repeats, method="versions alternated in one call, median of repeats, spread = (max - min) / median, device events")

    # ---- one BiLSTM layer
    B, T, P = a.batch, int(a.seconds * 100) // 2, 512
    g = torch.Generator().manual_seed(0)
    xg = (torch.randn(B, T, 8 * P, generator=g) * 0.7).to(torch.bfloat16).to(dev)
    rk = (torch.randn(2, P, 4 * P, generator=g) / np.sqrt(P)).to(torch.bfloat16).to(dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    xg0, xg1 = xg[:, :, :4 * P].contiguous(), xg[:, :, 4 * P:].flip(1).contiguous()
    gates = torch.empty(B, T, 4 * P, dtype=torch.bfloat16, device=dev)
    cseq = torch.empty(B, T, P, dtype=torch.float32, device=dev)
    hseq, yseq = (torch.empty(B, T, P, dtype=torch.bfloat16, device=dev) for _ in range(2))
    sync = K.lstm_persist_sync(dev)

    def two_launches():
        K.lstm_persist_fwd(xg0, rk[0], None, None, lens, gates, cseq, hseq, yseq, sync)
        K.lstm_persist_fwd(xg1, rk[1], None, None, lens, gates, cseq, hseq, yseq, sync)

    def step_route():
        prev = K.lstm_set_persist(0)
        try:
            K.lstm_infer_fwd(xg, rk, lens, ndir=2)
        finally:
            K.lstm_set_persist(prev)

    r = alternated({"one_launch_two_directions": lambda: K.lstm_infer_fwd(xg, rk, lens, ndir=2), "two_sequential_persist_launches": two_launches},
                   a.warmup, a.repeats)
    r.update(alternated({"per_step_route": step_route}, 1, 3))
    one, two = r["one_launch_two_directions"], r["two_sequential_persist_launches"]
    r["speedup_over_two_launches"] = two["median_ms"] / one["median_ms"]
    r["faster_by_more_than_the_spread"] = bool(two["median_ms"] - one["median_ms"] > max(one["spread"] * one["median_ms"], two["spread"] * two["median_ms"]))
    r["us_per_step_one_launch"] = one["median_ms"] * 1e3 / T
    r["shape"] = dict(B=B, T=T, P=P)
    out["bilstm_layer_bf16"] = r
    print(json.dumps({"bilstm_layer_bf16": r}), flush=True)

    # ---- conv module and whole recognize, per type
    for dtype, prec in ((torch.bfloat16, "bf16"), (torch.float32, "f32")):
        model = DeepSpeech2CTC(configs.deepspeech2(vocab_size=29), dev, dtype=dtype, seed=0)
        model.decode_precision = prec
        feats, flen = model.frontend(sig.to(dev), [n] * a.batch)
        base = conv1d_baseline(model, feats)
        torch.cuda.synchronize()
        rc = alternated({"conv2d_two_launches": lambda: model.conv_module_fwd(feats), "conv1d_per_frequency_baseline": base}, a.warmup, a.repeats)
        rc["baseline_over_kernel"] = rc["conv1d_per_frequency_baseline"]["median_ms"] / rc["conv2d_two_launches"]["median_ms"]
        flop = 0
        for (kh, kw, ci, co, st, sf, Fi, Fo), Tn in zip(model.cfg.conv_shapes(), (feats.shape[1], -(-feats.shape[1] // model.cfg.conv_strides[0][0]))):
            flop += 2 * kh * kw * ci * co * a.batch * (-(-Tn // st)) * Fo
        rc["flop"] = flop
        rc["tflops"] = flop / (rc["conv2d_two_launches"]["median_ms"] / 1e3) / 1e12
        out[f"conv_module_{prec}"] = rc
        print(json.dumps({f"conv_module_{prec}": rc}), flush=True)
        rr = alternated({"recognize": lambda: model.recognize(x), "encoder": lambda: model.encoder_fwd(feats, flen, False, None)}, 1,
                        max(3, a.repeats // 2))
        rr["recognize_rtf"] = rr["recognize"]["median_ms"] / 1e3 / audio_s
        out[f"recognize_{prec}"] = rr
        print(json.dumps({f"recognize_{prec}": rr}), flush=True)
        del model
        torch.cuda.empty_cache()
    out["f32_twin_slowdown_of_recognize"] = out["recognize_f32"]["recognize"]["median_ms"] / out["recognize_bf16"]["recognize"]["median_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
