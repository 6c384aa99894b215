"""One iteration of the greedy transducer search, stage by stage, in torch on the CPU: what csrc/decode_step.hip and the bookkeeping
kernel of csrc/decode.hip must compute.  float64 by default (the reference the GPU tests hold the kernels to); in float32 a loop of
`step` + `update` reproduces oracle/conformer_ref.py's recognize_batch / recognize_single bit for bit (tests/test_decode_oracle.py).

Follows  models/transducer/base_transducer.py:437-464   Transducer.call_next: embedding -> LSTM cell -> LayerNorm -> joint -> log_softmax
         models/transducer/base_transducer.py:496-575   recognize_batch (mode 0)
         models/transducer/base_transducer.py:577-712   recognize_single (mode 1); mode 2 is its rule for every row of a batch on its own

W maps the parameter names of ParamStore.export_keras ("pred/emb", "pred/lstm/k|rk|b", "pred/ln/g|b", "joint/pred/w|b",
"joint/vocab/w|b") to tensors.  `encj` [B, T, J] is the encoder output AFTER the joint's encoder projection, as the device holds it."""
import numpy as np
import torch
import torch.nn.functional as F

LN_EPS = 1e-3


def _t(a, dtype=None):
    a = torch.as_tensor(a)
    return a if dtype is None else a.to(dtype)


def frame_of(nframes, frame_idx, T):
    """the encoder frame a row reads: clamp(min(frame_idx, nframes - 1), 0, T - 1) (a finished row of mode 0 re-reads its last frame)"""
    nframes, frame_idx = _t(nframes).long().view(-1), _t(frame_idx).long().view(-1)
    return torch.minimum(frame_idx, nframes - 1).clamp(0, T - 1)


def step(W, prev_tok, h, c, encj, nframes, frame_idx, T, ln=True, dtype=torch.float64, h_new=None, z=None):
    """(c_new [B, P], h_new [B, P], z [B, J], logits [B, V]) of Transducer.call_next in `dtype`.  `h_new` / `z`, when given, replace the
    stage's own result as the input of the later stages (the returned c_new / h_new are still computed from h, c)."""
    w = {k: v.to(dtype) for k, v in W.items() if k.startswith(("pred/", "joint/pred/", "joint/vocab/"))}
    h, c, encj = _t(h, dtype), _t(c, dtype), _t(encj, dtype)
    B = h.shape[0]
    # keras LSTMCell, gates i, f, c, o: x @ kernel + bias, + h @ recurrent_kernel
    e = w["pred/emb"][_t(prev_tok).long().view(B, 1)]  # [B, 1, E]
    xg = e @ w["pred/lstm/k"] + w["pred/lstm/b"]
    pre = xg[:, 0] + h @ w["pred/lstm/rk"]
    i, f, g, o = pre.chunk(4, dim=-1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c_new = f * c + i * g
    h_own = o * torch.tanh(c_new)
    y = (h_own if h_new is None else _t(h_new, dtype))[:, None, :]  # [B, 1, P]
    if ln:
        y = F.layer_norm(y, (y.shape[-1],), w["pred/ln/g"], w["pred/ln/b"], LN_EPS)
    p = y @ w["joint/pred/w"] + w["joint/pred/b"]
    cur = encj[torch.arange(B), frame_of(nframes, frame_idx, T)][:, None, :]  # [B, 1, J]
    z_own = torch.tanh(cur[:, :, None, :] + p[:, None, :, :])  # TransducerJointMerge "add" + tanh, [B, 1, 1, J]
    zz = z_own if z is None else _t(z, dtype).view(B, 1, 1, -1)
    logits = zz @ w["joint/vocab/w"] + w["joint/vocab/b"]
    return c_new, h_own, z_own.view(B, -1), logits.view(B, -1)


def active(mode, nframes, frame_idx, tok_idx, max_tokens):
    """the while_loop condition: mode 0 stops once every row sits on its last frame or every row has filled its buffer; modes 1 and 2
    run while any row has a frame left"""
    nframes, frame_idx, tok_idx = (np.asarray(a).astype(np.int64).reshape(-1) for a in (nframes, frame_idx, tok_idx))
    if mode == 0:
        return not (bool((frame_idx >= nframes - 1).all()) or bool((tok_idx >= max_tokens - 1).all()))
    return bool((frame_idx < nframes).any())


def new_state(mode, B, P, nframes, max_tokens, blank=0, dtype=np.float32):
    """the search's initial state: tokens, counters and a zero decoder state"""
    return dict(nframes=np.asarray(nframes, np.int64).reshape(B).copy(), frame_idx=np.zeros(B, np.int64), prev_tok=np.full(B, blank, np.int64),
                tok_idx=np.full(B, 1 if mode == 0 else -1, np.int64), tokens=np.full((B, max(max_tokens, 1)), blank, np.int64),
                per_frame=(np.zeros(max(int(np.asarray(nframes).reshape(-1)[0]), 1), np.int64) if mode == 1 else np.zeros(B, np.int64)),
                h=np.zeros((B, P), dtype), c=np.zeros((B, P), dtype))


def log_softmax_f32(logits):
    return torch.log_softmax(_t(logits, torch.float32), -1).numpy()


def update(mode, logits, st, h_new, c_new, max_tokens, blank=0, max_tokens_per_frame=3):
    """One iteration of the bookkeeping on a copy of `st` (dict of NumPy arrays: nframes, frame_idx, prev_tok, tok_idx, tokens [B,
    max_tokens], per_frame, h, c).  The symbol of a row is np.argmax (first maximal index, as tf.argmax) of the f32 log-softmax."""
    st = {k: np.array(v, copy=True) for k, v in st.items()}
    cur = np.argmax(log_softmax_f32(logits), axis=-1)
    h_new, c_new = np.asarray(h_new), np.asarray(c_new)
    B = cur.shape[0]
    nframes, frame_idx, prev_tok, tok_idx, tokens, per_frame = (st[k] for k in ("nframes", "frame_idx", "prev_tok", "tok_idx", "tokens", "per_frame"))
    for b in range(B):
        tok = int(cur[b])
        if mode == 0:  # recognize_batch: column 0 collects the blanks, symbols go to columns 2.., the last column is overwritten
            eq_blank = tok == blank or tok_idx[b] >= max_tokens or frame_idx[b] > nframes[b]
            if eq_blank:
                tokens[b, 0] = blank
                frame_idx[b] += 1
                continue
            tok_idx[b] = min(tok_idx[b] + 1, max_tokens - 1)
            tokens[b, tok_idx[b]] = tok
        elif mode == 1:  # recognize_single: at most max_tokens_per_frame symbols on a frame; tokens[token_index] is re-written every iteration
            assert B == 1
            fi = int(frame_idx[0])
            if tok != blank:
                per_frame[fi] += 1
            if tok == blank or per_frame[fi] >= max_tokens_per_frame:
                frame_idx[0] = fi + 1
            if tok != blank:
                tok_idx[0] += 1
                prev_tok[0] = tok
            if tok_idx[0] >= 0:
                tokens.reshape(-1)[tok_idx[0]] = prev_tok[0]
            if tok == blank:
                continue
        else:  # the rule of mode 1 per row: per_frame[b] counts the symbols of the row's current frame; a finished row stands still
            if not frame_idx[b] < nframes[b]:
                continue
            nf = per_frame[b] + (tok != blank)
            advance = tok == blank or nf >= max_tokens_per_frame
            per_frame[b] = 0 if advance else nf
            if advance:
                frame_idx[b] += 1
            if tok == blank:
                continue
            if tok_idx[b] + 1 < max_tokens:  # a symbol past the buffer is dropped; the decoder still moves on
                tok_idx[b] += 1
                tokens[b, tok_idx[b]] = tok
        # a symbol was emitted: the decoder takes the new state
        prev_tok[b] = tok
        st["h"][b] = h_new[b]
        st["c"][b] = c_new[b]
    return st


def search(mode, W, encj, nframes, ln=True, dtype=torch.float64, blank=0, max_tokens_per_frame=3, max_tokens=None, trace=None):
    """the whole greedy search as a loop of active / step / update; returns the final state.  `trace` (a list) receives, per iteration,
    (top-1 minus top-2 log-probability per row [B], the rows whose decision counted [B] bool)."""
    encj = _t(encj, dtype)
    B, T, _ = encj.shape
    P = W["pred/lstm/rk"].shape[0]
    if max_tokens is None:
        max_tokens = int(np.asarray(nframes).reshape(-1)[0]) * max_tokens_per_frame if mode == 1 else 2 * T + 1
    npdt = np.float64 if dtype == torch.float64 else np.float32
    st = new_state(mode, B, P, nframes, max_tokens, blank, npdt)
    for _ in range(T + max_tokens + 2):  # (the product's cap on the reference's unbounded loop)
        if not active(mode, st["nframes"], st["frame_idx"], st["tok_idx"], max_tokens):
            break
        c_new, h_new, _, logits = step(W, st["prev_tok"], st["h"], st["c"], encj, st["nframes"], st["frame_idx"], T, ln, dtype)
        if trace is not None:
            top = torch.log_softmax(logits, -1).topk(2, -1).values
            counted = (st["frame_idx"] < st["nframes"]) if mode else ((st["tok_idx"] < max_tokens) & (st["frame_idx"] <= st["nframes"]))
            trace.append(((top[:, 0] - top[:, 1]).numpy(), counted.copy()))
        st = update(mode, logits, st, h_new.numpy(), c_new.numpy(), max_tokens, blank, max_tokens_per_frame)
    return st
