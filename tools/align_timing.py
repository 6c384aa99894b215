"""Forced alignment at the bench's shape (Conformer-M, bf16 model, 32 x 10 s, V = 1000, 64 labels per utterance).
  python tools/align_timing.py [--reps N] [--out FILE.json]
Timed with HIP events after warm-up, [median, min, max] ms over N repetitions, all on ONE batch:
  encode                 log-mel + encoder (inference mode, bf16)
  align_encoded          prediction network + packed joint + vocabulary product + log-probabilities + walk + back-trace, from encoder output
  align                  encode + align_encoded (model.align(data, precision="bf16"))
  loss_forward           loss_and_backward(training=False, want_backward=False): the same passes with the loss's two-sided lattice
                         walk in place of the Viterbi walk (it exists unchanged before the alignment was added)
  walk_only              kernels.rnnt_align_lattice on a random dense lattice [B, T', 65] with the same lengths: walk + back-trace alone
  ctc_walk_only          kernels.ctc_align(normalized=True) on random log-probabilities [B, T', V]: walk + back-trace alone
and which route the alignment took (statistics only / statistics beside logits / materialised logits)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())

import numpy as np
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.schemas import TrainData, TrainInput, TrainLabel

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda", 0)
model = ConformerTransducer(configs.conformer_m(), dev, dtype=torch.bfloat16, seed=0)
rng = np.random.default_rng(0)
B, secs, U = 32, 10.0, 64
n = int(secs * 16000)
V = model.cfg.vocab_size
sig = torch.from_numpy(np.clip(rng.standard_normal((B, n)).astype(np.float32) * 0.1, -1, 1)).to(dev)
slen = torch.full((B,), n, dtype=torch.int32)
labels = torch.from_numpy(rng.integers(1, V, (B, U)).astype(np.int32))
llen = torch.from_numpy(rng.integers(U // 2, U + 1, B).astype(np.int32))
preds = torch.cat([torch.zeros(B, 1, dtype=torch.int32), labels], 1)
data = TrainData(TrainInput(sig, slen, preds, llen + 1), TrainLabel(labels, llen))
enc, elen = model.encode(sig, slen, "bf16")
T = enc.shape[1]


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


# which route align_encoded takes at this shape
route = []
real_gemm, real_plain = K.gemm, K.rnnt_align


def spy_gemm(A, Bm, out, *a, **k):
    r = real_gemm(A, Bm, out, *a, **k)
    if k.get("lse") is not None:
        route.append("statistics only (no logits)" if out is None else "statistics beside materialised logits")
    return r


def spy_plain(*a, **k):
    route.append("materialised logits")
    return real_plain(*a, **k)


K.gemm, K.rnnt_align = spy_gemm, spy_plain
out = model.align_encoded(enc, elen, preds, labels, llen)
K.gemm, K.rnnt_align = real_gemm, real_plain
torch.cuda.synchronize()

tl = torch.tensor([min(int(v), T) for v in elen], dtype=torch.int32, device=dev)
ul = llen.to(dev)
g = torch.Generator(device=dev).manual_seed(1)
bl = -torch.rand(B, T, U + 1, generator=g, device=dev) * 8
tr = -torch.rand(B, T, U + 1, generator=g, device=dev) * 8
lp = torch.log_softmax(torch.randn(B, T, V, generator=g, device=dev), -1)
lab_d = labels.to(dev)
ctl = torch.maximum(tl, 2 * ul + 1).clamp(max=T)

res = {
    "encode_ms": timed(lambda: model.encode(sig, slen, "bf16")),
    "align_encoded_ms": timed(lambda: model.align_encoded(enc, elen, preds, labels, llen)),
    "align_ms": timed(lambda: model.align(data, precision="bf16")),
    "loss_forward_ms": timed(lambda: model.loss_and_backward(data, False, (None, None), want_backward=False)),
    "walk_only_ms": timed(lambda: K.rnnt_align_lattice(bl, tr, ul, tl)),
    "ctc_walk_only_ms": timed(lambda: K.ctc_align(lp, lab_d, ul, ctl, normalized=True)),
}
res["align_over_loss_forward"] = round(res["align_ms"][0] / res["loss_forward_ms"][0], 3)
frames = out.frames.cpu().numpy()
res["route"] = route
res["finite_scores"] = int(torch.isfinite(out.scores).sum())
res["mean_first_last_label_frame"] = [round(float(np.mean([f[0] for f, u in zip(frames, llen.tolist()) if u])), 1),
                                      round(float(np.mean([f[u - 1] for f, u in zip(frames, llen.tolist()) if u])), 1)]
out_json = {"shape": f"conformer_m bf16, {B} x {secs:.0f} s, T' = {T}, U = {U} (32..64 labels per utterance), J = {model.cfg.joint_dim}, V = {V}",
            "results": res,
            "note": "[median, min, max] ms over repetitions, HIP events, one batch; see the tool's docstring for what each row covers"}
print(json.dumps(out_json, indent=1))
if args.out:
    with open(args.out, "w") as f:
        json.dump(out_json, f, indent=1)
