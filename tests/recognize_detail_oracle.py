"""What recognize_detailed must report, on the CPU: a recorder around tests/decode_oracle.py's step / update (the transducer's greedy search
with, per emitted symbol, the encoder frame of the decision, the symbol's log-probability and the entropy of the decision's distribution)
and a NumPy CTC greedy decoder with the span of every token.  float64 by default: the reference the GPU tests hold the kernels to.

The recorder does not decide anything itself: the symbol and every counter come from decode_oracle.update, and a symbol counts as written
where update's own result says so (mode 0: the row did not advance its frame; modes 1 and 2: tok_idx moved)."""
import json
import os

import numpy as np
import torch

import decode_oracle as DO

BAR = dict(rtol=1e-4, atol=1e-5)  # the project's single-layer f32 bar (tests/test_decode_step_gpu.py)
PARITY_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "recognize_detail_parity.json")


def ratio(got, ref, n=1):
    """worst |got - ref| / (n atol + rtol |ref|) against the bar (n: the number of terms summed into each value); 0 for empty input"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    return float((np.abs(got - ref) / (np.asarray(n, np.float64) * BAR["atol"] + BAR["rtol"] * np.abs(ref))).max())


def write_parity(section, cases):
    """merge one test module's worst ratios into profiles/recognize_detail_parity.json"""
    doc = {}
    if os.path.exists(PARITY_FILE):
        with open(PARITY_FILE) as f:
            doc = json.load(f)
    doc["what"] = "worst |device - float64| / (n atol + rtol |float64|) of the token log-probabilities and entropies (tests/test_decode_detail_gpu.py, tests/test_ctc_detail_gpu.py)"
    doc["bar"] = BAR
    doc[section] = cases
    os.makedirs(os.path.dirname(PARITY_FILE), exist_ok=True)
    with open(PARITY_FILE, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def entropy(lsm):
    """H = -sum_v p_v log p_v over the last axis of a log-softmax; a class with p_v == 0 (log p_v = -inf included) contributes 0"""
    p = torch.exp(lsm)
    return -torch.where(p > 0, p * lsm, torch.zeros_like(lsm)).sum(-1)


def new_detail(tokens):
    """the caller-initialised detail buffers, shaped like `tokens`"""
    return dict(frames=np.full(tokens.shape, -1, np.int64), logp=np.zeros(tokens.shape, np.float64), entropy=np.zeros(tokens.shape, np.float64))


def update_detail(mode, logits, st, det, h_new, c_new, max_tokens, T, blank=0, max_tokens_per_frame=3, dtype=torch.float64):
    """One iteration of decode_oracle.update plus the detail bookkeeping on copies of `st` and `det`; the log-softmax is taken in `dtype` of
    the logits as given.  Returns (st, det, written [B] bool)."""
    lsm = torch.log_softmax(torch.as_tensor(logits).to(dtype), -1)
    H = entropy(lsm).numpy()
    frame = DO.frame_of(st["nframes"], st["frame_idx"], T).numpy()
    new = DO.update(mode, logits, st, h_new, c_new, max_tokens, blank, max_tokens_per_frame)
    det = {k: np.array(v, copy=True) for k, v in det.items()}
    B = lsm.shape[0]
    written = np.zeros(B, bool)
    for b in range(B):
        if mode == 0:
            written[b] = new["frame_idx"][b] == st["frame_idx"][b]  # a blank (forced or not) advances the frame, a symbol does not
        else:
            written[b] = new["tok_idx"][b] != st["tok_idx"][b]  # (mode 2: a symbol dropped past the buffer leaves tok_idx alone)
        if written[b]:
            ti = int(new["tok_idx"][b])
            cur = int(new["tokens"][b, ti]) if mode != 1 else int(new["tokens"].reshape(-1)[ti])
            idx = (b, ti) if mode != 1 else (0, ti)
            assert cur != blank and cur == new["prev_tok"][b]
            det["frames"][idx] = frame[b]
            det["logp"][idx] = float(lsm[b, cur])
            det["entropy"][idx] = H[b]
    return new, det, written


def search(mode, W, encj, nframes, ln=True, dtype=torch.float64, blank=0, max_tokens_per_frame=3, max_tokens=None, trace=None):
    """decode_oracle.search with the recorder: returns (final state, detail buffers).  `trace` receives, per iteration, (top-1 minus top-2
    log-probability per row, the rows whose decision counted), as decode_oracle.search's."""
    encj = torch.as_tensor(encj).to(dtype)
    B, T, _ = encj.shape
    P = W["pred/lstm/rk"].shape[0]
    if max_tokens is None:
        max_tokens = int(np.asarray(nframes).reshape(-1)[0]) * max_tokens_per_frame if mode == 1 else 2 * T + 1
    st = DO.new_state(mode, B, P, nframes, max_tokens, blank, np.float64 if dtype == torch.float64 else np.float32)
    det = new_detail(st["tokens"])
    for _ in range(T + max_tokens + 2):
        if not DO.active(mode, st["nframes"], st["frame_idx"], st["tok_idx"], max_tokens):
            break
        c_new, h_new, _, logits = DO.step(W, st["prev_tok"], st["h"], st["c"], encj, st["nframes"], st["frame_idx"], T, ln, dtype)
        if trace is not None:
            top = torch.log_softmax(logits, -1).topk(2, -1).values
            counted = (st["frame_idx"] < st["nframes"]) if mode else ((st["tok_idx"] < max_tokens) & (st["frame_idx"] <= st["nframes"]))
            trace.append(((top[:, 0] - top[:, 1]).numpy(), counted.copy()))
        st, det, _ = update_detail(mode, logits, st, det, h_new.numpy(), c_new.numpy(), max_tokens, T, blank, max_tokens_per_frame, dtype)
    return st, det


def ctc_greedy_detail(logits, logit_len, blank=0, dtype=np.float64):
    """tf.nn.ctc_greedy_decoder(merge_repeated=True) over logits [B, T, V] with spans -> dict: tokens [B, T] (blank padded), tokens_len [B],
    starts / ends [B, T] (-1 past tokens_len; token i holds the frames [starts, ends) of its run of equal arg-max classes), logp [B, T]
    (the frames' maximal log-softmax summed over the run), entropy [B, T] (mean frame entropy of the run), nframes [B, T] (ends - starts,
    0 past tokens_len), score [B] (sum of the maxima over all valid frames), amax [B, T] (first maximal index per frame)."""
    x = np.asarray(logits, dtype)
    B, T, V = x.shape
    lsm = torch.log_softmax(torch.from_numpy(x), -1)
    H = entropy(lsm).numpy()
    lsm = lsm.numpy()
    amax = np.argmax(x, -1)
    out = dict(tokens=np.full((B, T), blank, np.int64), tokens_len=np.zeros(B, np.int64), starts=np.full((B, T), -1, np.int64),
               ends=np.full((B, T), -1, np.int64), logp=np.zeros((B, T), dtype), entropy=np.zeros((B, T), dtype), nframes=np.zeros((B, T), np.int64),
               score=np.zeros(B, dtype), amax=amax)
    for b in range(B):
        Tl = min(max(int(logit_len[b]), 0), T)
        n, t = 0, 0
        while t < Tl:
            c, e = int(amax[b, t]), t + 1
            while e < Tl and amax[b, e] == c:
                e += 1
            if c != blank:
                out["tokens"][b, n], out["starts"][b, n], out["ends"][b, n], out["nframes"][b, n] = c, t, e, e - t
                out["logp"][b, n] = lsm[b, t:e, c].sum(dtype=dtype)
                out["entropy"][b, n] = H[b, t:e].mean(dtype=dtype)
                n += 1
            t = e
        out["tokens_len"][b] = n
        out["score"][b] = lsm[b, np.arange(Tl), amax[b, :Tl]].sum(dtype=dtype)
    return out
