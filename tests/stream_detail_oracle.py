"""What tfasr_ctc_greedy_decode_carry_detail must report, on the CPU: a NumPy CTC greedy decoder that takes one chunk of frames per call
and carries, per stream, what an unfinished token needs.  float64 by default: the reference tests/test_ctc_carry_detail_gpu.py holds the
kernel to.  tests/test_stream_detail_oracle.py pins it against recognize_detail_oracle.ctc_greedy_detail on the whole buffer.

The frame values (arg-max, its log-softmax, the entropy) are those of recognize_detail_oracle: one torch.log_softmax per frame row.  The
state keeps the open token's frame values and every frame's log-probability as lists and reduces them with the NumPy calls the one-shot
decoder uses (sum / mean over the run), so the two agree to the bit however the buffer is cut; the kernel keeps running f32 sums instead,
which is the same thing up to the rounding the GPU test's bar allows.

Output layout of chunk(): the kernel's.  Row b, C + 1 columns: column 0 = the token that was open on entry (starts = -1: none), columns
1 .. tokens_len[b] = the tokens that start in this chunk; ends = -1 and the values over the frames so far for a token still open;
unoccupied columns blank / -1 / -1 / 0 / 0.  Frames are global: counted from the stream's reset."""
import numpy as np
import torch

import recognize_detail_oracle as RD


def new_state(B):
    """per stream: previous class (-1: none), frames seen, the open token (None, or its class / first frame / frame values), all frames'
    log-probabilities"""
    return [dict(prev=-1, seen=0, open=None, lps=[]) for _ in range(B)]


def reset(state, rows):
    for b in rows:
        state[b] = new_state(1)[0]


def score(state, dtype=np.float64):
    return np.array([np.asarray(s["lps"], dtype).sum(dtype=dtype) if s["lps"] else 0.0 for s in state], dtype)


def _values(tok, dtype):
    return np.asarray(tok["lp"], dtype).sum(dtype=dtype), np.asarray(tok["ent"], dtype).mean(dtype=dtype)


def chunk(logits, logit_len, state, final=None, blank=0, dtype=np.float64):
    """One chunk logits [B, C, V] (C >= 1), logit_len [B] valid frames, final [B] flags (None: none set); `state` is updated in place
    (a row with no frames and no flag is left alone) -> dict of tokens / starts / ends [B, C + 1] int64, tokens_len [B], logp / entropy
    [B, C + 1], nframes [B, C + 1] (frames summed into each value so far)."""
    x = np.asarray(logits, dtype)
    B, C, V = x.shape
    lsm = torch.log_softmax(torch.from_numpy(x), -1)
    H = RD.entropy(lsm).numpy()
    lsm = lsm.numpy()
    amax = np.argmax(x, -1)
    W = C + 1
    out = dict(tokens=np.full((B, W), blank, np.int64), tokens_len=np.zeros(B, np.int64), starts=np.full((B, W), -1, np.int64),
               ends=np.full((B, W), -1, np.int64), logp=np.zeros((B, W), dtype), entropy=np.zeros((B, W), dtype), nframes=np.zeros((B, W), np.int64))

    def put(b, col, tok, end):
        out["tokens"][b, col], out["starts"][b, col], out["ends"][b, col] = tok["cls"], tok["start"], end
        out["logp"][b, col], out["entropy"][b, col] = _values(tok, dtype)
        out["nframes"][b, col] = len(tok["lp"])

    for b in range(B):
        s = state[b]
        Tl = min(max(int(logit_len[b]), 0), C)
        fin = final is not None and bool(final[b])
        if Tl == 0 and not fin:
            if s["open"] is not None:
                put(b, 0, s["open"], -1)
            continue
        n, col = 0, 0
        for t in range(Tl):
            c, g = int(amax[b, t]), s["seen"] + t
            if c != s["prev"]:
                if s["open"] is not None:
                    put(b, col, s["open"], g)
                    s["open"] = None
                if c != blank:
                    n += 1
                    col = n
                    s["open"] = dict(cls=c, start=g, lp=[], ent=[])
            s["lps"].append(lsm[b, t, c])
            if s["open"] is not None:
                s["open"]["lp"].append(lsm[b, t, c])
                s["open"]["ent"].append(H[b, t])
            s["prev"] = c
        s["seen"] += Tl
        if s["open"] is not None:
            put(b, col, s["open"], s["seen"] if fin else -1)
            if fin:
                s["open"] = None
        out["tokens_len"][b] = n
    return out


def closed(out, b):
    """the tokens of row b that CLOSED in this call, in order: (class, start, end, logp, entropy) tuples"""
    return [(int(out["tokens"][b, i]), int(out["starts"][b, i]), int(out["ends"][b, i]), out["logp"][b, i], out["entropy"][b, i])
            for i in range(out["tokens"].shape[1]) if out["starts"][b, i] >= 0 and out["ends"][b, i] >= 0]


def run_split(logits, lens, cuts, blank=0, dtype=np.float64, final=True):
    """Feed logits [B, T, V] with per-row lengths `lens` in consecutive chunks: cuts = a list of [B] per-row frame counts per call (0
    allowed; a call's chunk is as wide as its longest row, at least 1).  After the calls one more with no frames and the final flag, if
    `final`.  -> (per row the closed tokens of all calls in order, the state, the per-call outputs)."""
    x = np.asarray(logits)
    B, T, V = x.shape
    state, pos, outs = new_state(B), [0] * B, []
    toks = [[] for _ in range(B)]
    calls = [(list(c), None) for c in cuts] + ([([0] * B, [1] * B)] if final else [])
    for take, fin in calls:
        take = [min(int(n), int(lens[b]) - pos[b]) for b, n in enumerate(take)]
        C = max(max(take), 1)
        buf = np.zeros((B, C, V), x.dtype)
        for b in range(B):
            buf[b, :take[b]] = x[b, pos[b]:pos[b] + take[b]]
            pos[b] += take[b]
        out = chunk(buf, take, state, fin, blank, dtype)
        outs.append(out)
        for b in range(B):
            toks[b] += closed(out, b)
    return toks, state, outs
