"""CTC beam search at the bench's CTC shape (Conformer-CTC S, 32 x 10 s, V = 1000, beam 10): host routine vs device search.
  python tools/ctc_beam_timing.py [reps]
Regions timed with HIP events after warm-up, median of `reps` repetitions: the host search (logits copied to host memory +
tfasr_ctc_beam_search_host, the default of recognize_beam), the device search (tfasr_ctc_beam_search: frame pass + search pass),
and log-mel + encoder + device search (recognize_beam(device_search=True)).  Also reports whether the two searches agree."""
import os
import sys

sys.path.insert(0, os.getcwd())
import json

import numpy as np
import torch

from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.ctc_model import ConformerCTC
from tensorflowasr_amd.schemas import PredictInput

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
dev = torch.device("cuda", 0)
model = ConformerCTC(configs.conformer_ctc_s(), dev, dtype=torch.bfloat16, seed=0)
rng = np.random.default_rng(0)
B, n, W = 32, 160000, 10
sig = torch.from_numpy(np.clip(rng.standard_normal((B, n)).astype(np.float32) * 0.1, -1, 1)).to(dev)
inp = PredictInput(sig, torch.full((B,), n, dtype=torch.int32))
logits, elen = model._infer_logits(inp)
ln = torch.tensor(elen, dtype=torch.int32)
ln_dev = ln.to(dev)


def timed(fn, reps=REPS, warmup=2):
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
    return float(np.median(ms)), float(min(ms)), float(max(ms))


host = timed(lambda: K.ctc_beam_search(logits, ln, beam_width=W), reps=max(3, REPS // 3))
devs = timed(lambda: K.ctc_beam_search_device(logits, ln_dev, beam_width=W))
full = timed(lambda: model.recognize_beam(inp, beam_width=W, device_search=True))
ht, hn, _ = K.ctc_beam_search(logits, ln, beam_width=W)
dt, dn, _ = K.ctc_beam_search_device(logits, ln_dev, beam_width=W)
same = bool(torch.equal(dt[:, 0].cpu(), ht) and torch.equal(dn[:, 0].cpu(), hn))
print(json.dumps({"shape": f"conformer_ctc_s {B} x 10 s, T = {logits.shape[1]}, V = {logits.shape[2]}, beam {W}",
                  "host_search_ms": [round(v, 3) for v in host], "device_search_ms": [round(v, 3) for v in devs],
                  "encoder_plus_device_search_ms": [round(v, 3) for v in full], "speedup_search": round(host[0] / devs[0], 1),
                  "tokens_equal_host": same, "note": "[median, min, max] over repetitions, HIP events"}))
