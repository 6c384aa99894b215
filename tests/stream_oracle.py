"""Chunk-by-chunk restatement of the f64 oracle (oracle/conformer_ref.py) with carried state: what the streaming session must
compute.  tests/test_stream_oracle.py proves it equal to the oracle's offline run of the utterance alone; the GPU tests compare the
kernels and the session against it."""
import math
import os

import numpy as np
import torch

from oracle import conformer_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STREAM_OVER = dict(chunk_size=2, history_size=4, convm_dw_norm="layer", sub_norm="layer")


def load_golden(name="conformer_streaming", dtype=torch.float64):
    z = np.load(os.path.join(GOLD, f"wiring_{name}.npz"))
    W = {k[2:]: torch.from_numpy(z[k]).to(dtype) for k in z.files if k.startswith("W/")}
    for k in z.files:  # the eval call of the golden ran on the moving statistics one training call left behind
        if k.startswith("after_train/"):
            W[k[len("after_train/"):]] = torch.from_numpy(z[k]).to(dtype)
    return z, W


def oracle_cfg(**over):
    cfg = R.conformer_config("tiny")
    cfg.update(over)
    return cfg


def offline_alone(sig, W, cfg):
    """(encoder output [T', d], features [T0, F]) of one utterance run alone through the offline oracle"""
    feat = R.log_mel(np.asarray(sig, np.float32)[None], cfg)
    flen = R.get_nframes([len(sig)])
    dt = W["enc/linear/w"].dtype
    x, _ = R.encoder(torch.from_numpy(feat).to(dt)[..., None], flen, W, cfg, training=False)
    return x[0], feat[0]


# ------------------------------------------------------------------------------------------- front end
def stream_logmel(sig, piece, cfg):
    """samples arrive `piece` at a time; a frame is emitted once its frame_length samples exist, the tail is zero padded at the end
    only; one raw sample is carried for the pre-emphasis.  -> [ceil(n / step), F] f32"""
    sr = cfg["sample_rate"]
    flen_, step = int(round(sr * cfg["frame_ms"] / 1000.0)), int(round(sr * cfg["stride_ms"] / 1000.0))
    coef = np.float32(cfg["preemphasis"])
    melw = R.mel_weight_matrix(cfg["num_feature_bins"], cfg["nfft"] // 2 + 1, sr, 0.0, 8000.0)
    win = R.hann_periodic(flen_)
    buf, prev, emitted, total, out = np.zeros(0, np.float32), None, 0, 0, []

    def emph(raw):
        y = np.empty_like(raw)
        y[1:] = raw[1:] - coef * raw[:-1]
        y[0] = raw[0] if prev is None else raw[0] - coef * prev
        return y

    def frames(e, nf):
        idx = np.arange(nf)[:, None] * step + np.arange(flen_)[None]
        spec = np.fft.rfft((e[idx] * win[None]).astype(np.float64), n=cfg["nfft"], axis=-1)
        power = np.square(np.abs(spec)).astype(np.float32)
        return np.log(power @ melw + np.float32(cfg["epsilon"])).astype(np.float32)

    sig = np.asarray(sig, np.float32)
    for pos in range(0, len(sig), piece):
        new = sig[pos:pos + piece]
        total += len(new)
        buf = np.concatenate([buf, new])
        nf = (len(buf) - flen_) // step + 1 if len(buf) >= flen_ else 0
        if nf > 0:
            out.append(frames(emph(buf), nf))
            prev, buf, emitted = buf[nf * step - 1], buf[nf * step:], emitted + nf
    nf = -(-total // step) - emitted
    if nf > 0:
        e = emph(buf) if len(buf) else buf
        out.append(frames(np.pad(e, (0, (nf - 1) * step + flen_ - len(e))), nf))
    return np.concatenate(out, 0)


# ------------------------------------------------------------------------------------------- kernels' arithmetic
def attn_chunk(q, k, v, kc, vc, p, u, vb, hist, C, scale):
    """q / k / v [n, H, dh] of the chunk's valid rows, kc / vc [nh, H, dh] the history in time order, p [hist + 2C - 1, H, dh] the
    projected table (row r <-> position hist + C - 1 - r) -> context [n, H, dh]"""
    n, nh = q.shape[0], kc.shape[0]
    keys, vals = torch.cat([kc, k], 0), torch.cat([vc, v], 0)
    content = torch.einsum("she,the->hts", keys, (q + u) * scale)
    posall = torch.einsum("rhe,the->htr", p, (q + vb) * scale)
    i = torch.arange(n)[:, None]
    j = torch.arange(nh + n)[None, :]
    r = hist + C - 1 - (nh + i - j)
    sc = content + torch.gather(posall, 2, r[None].expand(q.shape[1], n, nh + n))
    return torch.einsum("hts,she->the", torch.softmax(sc, -1), vals)


def glu_dwconv_chunk(a, state, w, b):
    """a [n, 2d], state [K-1, d] -> (y [n, d], new state)"""
    x, gate = a.chunk(2, -1)
    gg = torch.cat([state, x * torch.sigmoid(gate)], 0)
    Kk = w.shape[0]
    y = torch.stack([(gg[t:t + Kk] * w).sum(0) for t in range(a.shape[0])]) + b
    return y, gg[gg.shape[0] - (Kk - 1):]


def pos_table(hist, C, d, dtype=torch.float64):
    pos = torch.arange(hist + C - 1, -C, -1, dtype=torch.float32)
    return R.compute_sinusoid_position_encoding(pos, d, True).to(dtype)


class EncoderStream:
    """The encoder of ONE stream: feed(feature frames) whenever they arrive, flush() at the end; every call returns the encoder frames
    that became final ([0, d] if none).  Carries exactly the state table of DESIGN.md."""

    def __init__(self, W, cfg):
        self.W, self.cfg = W, cfg
        self.C, self.hist = cfg["chunk_size"], cfg["history_size"]
        H, dh, d, Kk = cfg["num_heads"], cfg["head_size"], cfg["dmodel"], cfg["kernel_size"]
        dt = W["enc/linear/w"].dtype
        self.dt = dt
        nb = cfg["num_blocks"]
        F1 = (cfg["num_feature_bins"] + 1) // 2
        self.pending = torch.zeros(0, cfg["num_feature_bins"], dtype=dt)
        self.fc = torch.zeros(2, cfg["num_feature_bins"], dtype=dt)
        self.cc = torch.zeros(2, F1, W["enc/sub/conv0/w"].shape[-1], dtype=dt)
        self.kc = [torch.zeros(0, H, dh, dtype=dt) for _ in range(nb)]
        self.vc = [torch.zeros(0, H, dh, dtype=dt) for _ in range(nb)]
        self.dw = [torch.zeros(Kk - 1, d, dtype=dt) for _ in range(nb)]
        pe = pos_table(self.hist, self.C, d, dt)
        self.p = [torch.einsum("rd,dhe->rhe", pe, W[f"enc/block{i}/mhsa/pos/w"]) + W[f"enc/block{i}/mhsa/pos/b"] for i in range(nb)]

    def _norm(self, x, name):
        W = self.W
        if self.cfg.get("sub_norm", "batch") == "layer":
            return R.layer_norm(x, W[name + "/g"], W[name + "/b"])
        return R.batch_norm_infer(x, W[name + "/g"], W[name + "/b"], W[name + "/mm"], W[name + "/mv"])

    def _sub(self, feat):
        W = self.W
        cat = torch.cat([self.fc, feat], 0)
        self.fc = cat[-2:]
        a1 = R.swish(self._norm(R.conv2d_causal_s2(cat[None, :, :, None], W["enc/sub/conv0/w"], W["enc/sub/conv0/b"]), "enc/sub/bn0"))[0, 1:]
        cat1 = torch.cat([self.cc, a1], 0)
        self.cc = cat1[-2:]
        a2 = R.swish(self._norm(R.conv2d_causal_s2(cat1[None], W["enc/sub/conv1/w"], W["enc/sub/conv1/b"]), "enc/sub/bn1"))[0, 1:]
        return a2.reshape(a2.shape[0], -1)

    def _chunk(self, feat):
        W, cfg = self.W, self.cfg
        x = self._sub(feat) @ W["enc/linear/w"] + W["enc/linear/b"]
        scale = 1.0 / math.sqrt(cfg["head_size"])
        for i in range(cfg["num_blocks"]):
            pfx = f"enc/block{i}/"
            x = R.ff_module(x[None], W, pfx + "ff1/", cfg["ffm_residual"])[0]
            m = pfx + "mhsa/"
            y = R.layer_norm(x, W[m + "ln/g"], W[m + "ln/b"])
            q, k, v = (torch.einsum("td,dhe->the", y, W[m + s + "/w"]) + W[m + s + "/b"] for s in "qkv")
            u_, v_ = (W[m + "u"], W[m + "v"]) if cfg.get("mhsam_use_attention_bias") else (W["enc/u"], W["enc/v"])
            ctx = attn_chunk(q, k, v, self.kc[i], self.vc[i], self.p[i], u_, v_, self.hist, self.C, scale)
            x = x + torch.einsum("the,hed->td", ctx, W[m + "o/w"]) + W[m + "o/b"]
            keys, vals = torch.cat([self.kc[i], k], 0), torch.cat([self.vc[i], v], 0)
            self.kc[i], self.vc[i] = (keys[-self.hist:], vals[-self.hist:]) if self.hist > 0 else (keys[:0], vals[:0])
            cp = pfx + "conv/"
            y = R.layer_norm(x, W[cp + "ln/g"], W[cp + "ln/b"])
            y, self.dw[i] = glu_dwconv_chunk(y @ W[cp + "pw1/w"] + W[cp + "pw1/b"], self.dw[i], W[cp + "dw/w"], W[cp + "dw/b"])
            if cfg.get("convm_dw_norm", "batch") == "layer":
                y = R.layer_norm(y, W[cp + "bn/g"], W[cp + "bn/b"])
            else:
                y = R.batch_norm_infer(y, W[cp + "bn/g"], W[cp + "bn/b"], W[cp + "bn/mm"], W[cp + "bn/mv"])
            x = x + R.swish(y) @ W[cp + "pw2/w"] + W[cp + "pw2/b"]
            x = R.ff_module(x[None], W, pfx + "ff2/", cfg["ffm_residual"])[0]
            x = R.layer_norm(x, W[pfx + "ln/g"], W[pfx + "ln/b"])
        return x

    def feed(self, feat):
        self.pending = torch.cat([self.pending, torch.as_tensor(feat).to(self.dt)], 0)
        out = [torch.zeros(0, self.cfg["dmodel"], dtype=self.dt)]
        n0 = 4 * self.C
        while self.pending.shape[0] >= n0:
            out.append(self._chunk(self.pending[:n0]))
            self.pending = self.pending[n0:]
        return torch.cat(out, 0)

    def flush(self):
        if self.pending.shape[0] == 0:
            return torch.zeros(0, self.cfg["dmodel"], dtype=self.dt)
        x, self.pending = self._chunk(self.pending), self.pending[:0]
        return x


def stream_encoder(feat, frames_per_call, W, cfg):
    s = EncoderStream(W, cfg)
    outs = [s.feed(feat[i:i + frames_per_call]) for i in range(0, feat.shape[0], frames_per_call)]
    return torch.cat(outs + [s.flush()], 0)


# ------------------------------------------------------------------------------------------- search
def recognize_single_carry(encoded, W, state=None, blank=0, max_tokens_per_frame=3, gaps=None):
    """R.recognize_single over encoded [1, n, d] continued from state = (prev_tok, h, c) -> (new tokens list, state).  gaps: optional
    list that receives best - second best log-probability of every decision."""
    P = W["pred/lstm/rk"].shape[0]
    if state is None:
        state = (torch.full((1, 1), blank, dtype=torch.long), torch.zeros(1, P, dtype=encoded.dtype), torch.zeros(1, P, dtype=encoded.dtype))
    prev_tok, h, c = state
    toks = []
    for frame in range(encoded.shape[1]):
        for _ in range(max_tokens_per_frame):
            lsm, hn, cn = R._call_next(encoded[:, frame:frame + 1], prev_tok, h, c, W)
            lp = lsm.view(-1)
            if gaps is not None:
                top = torch.topk(lp, 2).values
                gaps.append(float(top[0] - top[1]))
            cur = int(lp.argmax())
            if cur == blank:
                break
            toks.append(cur)
            prev_tok, h, c = torch.full((1, 1), cur, dtype=torch.long), hn, cn
    return toks, (prev_tok, h, c)


def ctc_greedy_carry(classes, last=-1, blank=0):
    out = []
    for cl in classes:
        if cl != last and cl != blank:
            out.append(int(cl))
        last = int(cl)
    return out, last


def oracle_decode(sig, W, cfg, max_tokens_per_frame=3):
    """f64 offline run of one utterance alone: (encoder frames [T', d], greedy tokens, smallest best - second-best log-probability gap
    over all decisions of the search)"""
    enc, _ = offline_alone(sig, W, cfg)
    gaps = []
    toks, _ = recognize_single_carry(enc[None], W, None, cfg.get("blank", 0), max_tokens_per_frame, gaps)
    return enc, toks, min(gaps)


def cfg_to_oracle(cfg):
    """the product's ConformerConfig as the oracle's dict"""
    import dataclasses

    return dataclasses.asdict(cfg)


def noise(seed, seconds, sample_rate=16000):
    """seeded noise utterances of the given lengths in seconds: list of f32 arrays"""
    rng = np.random.default_rng(seed)
    return [np.clip(rng.standard_normal(int(round(s * sample_rate))) * 0.1, -1, 1).astype(np.float32) for s in seconds]
