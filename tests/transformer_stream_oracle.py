"""Chunk-by-chunk restatement of the float64 Transformer oracle (tests/transformer_oracle.py) with carried state: what a streaming
session of the Transformer encoder must compute.  tests/test_transformer_stream_oracle.py proves it equal to the offline oracle's run of
the utterance alone; the GPU tests compare the kernels and the sessions against it.

State of one stream: the encoder frames seen so far, the last 2 feature frames, the last 2 rows of the first convolution block's
activation (after BatchNorm and ReLU), and per block one key ring and one value ring [history_size, H, dh] with frame f in slot
f % history_size.  A chunk of C = chunk_size encoder frames (4 C feature frames) sees the min(seen, history_size) frames in front of it and
itself (with the causal flag: itself up to the query row) - compute_streaming_mask's window for an utterance alone, where no row is padded."""
import math

import torch

import transformer_oracle as TO


def attn_chunk(q, k, v, hk, hv, scale, causal=False):
    """q / k / v [n, H, dh] of the chunk's valid rows, hk / hv [nh, H, dh] the history in time order -> context [n, H, dh]"""
    n, nh = q.shape[0], hk.shape[0]
    keys, vals = torch.cat([hk, k], 0), torch.cat([hv, v], 0)
    s = torch.einsum("the,she->hts", q * scale, keys)
    if causal:
        i, j = torch.arange(n)[:, None], torch.arange(nh + n)[None, :]
        s = s.masked_fill((j - nh > i)[None], -math.inf)
    return torch.einsum("hts,she->the", torch.softmax(s, -1), vals)


def ring_history(ring, seen, hist):
    """the min(seen, hist) newest frames of a ring [hist, ...] in time order"""
    nh = min(seen, hist)
    return torch.stack([ring[f % hist] for f in range(seen - nh, seen)]) if nh else ring[:0]


def ring_append(ring, rows, seen, hist):
    """rows r = 0 .. n-1 of a chunk are frames seen + r: into slot (seen + r) % hist, the last `hist` of them when n > hist"""
    n = rows.shape[0]
    for r in range(max(0, n - hist), n):
        ring[(seen + r) % hist] = rows[r]


class EncoderStream:
    """The encoder of ONE stream: feed(feature frames) whenever they arrive, flush() at the end; every call returns the encoder frames
    that became final ([0, d] if none)."""

    def __init__(self, W, cfg, dtype=torch.float64):
        self.W, self.cfg, self.dt = W, cfg, dtype
        self.C, self.hist = int(cfg.chunk_size), int(cfg.history_size)
        H, dh, F = int(cfg.num_heads), int(cfg.head_size), int(cfg.num_feature_bins)
        nb = int(cfg.num_blocks)
        self.seen = 0
        self.pending = torch.zeros(0, F, dtype=dtype)
        self.fc = torch.zeros(2, F, dtype=dtype)
        self.cc = torch.zeros(2, (F + 1) // 2, int(cfg.sub_filters[0]), dtype=dtype)
        self.kc = [torch.zeros(self.hist, H, dh, dtype=dtype) for _ in range(nb)]
        self.vc = [torch.zeros(self.hist, H, dh, dtype=dtype) for _ in range(nb)]

    def g(self, name):
        return self.W[name].to(self.dt)

    def _conv_block(self, x, i):
        """x [1, T, F, Cin] -> Conv2D 3x3 stride 2 causal -> [BatchNorm] -> ReLU"""
        p = f"enc/subsampling/block_{i}/"
        x = TO.conv2d_causal_s2(x, self.g(p + f"conv_{i}/w")) + self.g(p + f"conv_{i}/b")
        if self.cfg.sub_norm == "batch":
            bn = p + f"bn_{i}"
            x = (x - self.g(bn + "/mm")) / torch.sqrt(self.g(bn + "/mv") + TO.EPS) * self.g(bn + "/g") + self.g(bn + "/b")
        return torch.relu(x)

    def _sub(self, feat):
        """carry(2) ++ new rows through each causal stride-2 block: output 0 belongs to the previous chunk, outputs 1.. are the originals"""
        cat = torch.cat([self.fc, feat], 0)
        self.fc = cat[-2:]
        a1 = self._conv_block(cat[None, :, :, None], 0)[0, 1:]
        cat1 = torch.cat([self.cc, a1], 0)
        self.cc = cat1[-2:]
        a2 = self._conv_block(cat1[None], 1)[0, 1:]
        return a2.reshape(a2.shape[0], -1)

    def _block(self, x, i):
        cfg, g, p = self.cfg, self.g, f"enc/block_{i}"
        f, pre = float(cfg.residual_factor), cfg.norm_position == "pre"
        ln1 = lambda t: TO.layer_norm(t, g(p + "/ln_1/g"), g(p + "/ln_1/b"))
        ln2 = lambda t: TO.layer_norm(t, g(p + "/ln_2/g"), g(p + "/ln_2/b"))
        h = ln1(x) if pre else x
        q, k, v = (torch.einsum("td,dhe->the", h, g(f"{p}/mhsa/{n}/w")) + g(f"{p}/mhsa/{n}/b") for n in "qkv")
        hk, hv = ring_history(self.kc[i], self.seen, self.hist), ring_history(self.vc[i], self.seen, self.hist)
        ctx = attn_chunk(q, k, v, hk, hv, 1.0 / math.sqrt(int(cfg.head_size)), bool(cfg.use_attention_causal_mask))
        ring_append(self.kc[i], k, self.seen, self.hist)
        ring_append(self.vc[i], v, self.seen, self.hist)
        y = torch.einsum("the,hed->td", ctx, g(p + "/mhsa/o/w")) + g(p + "/mhsa/o/b")
        a = x + f * (y if pre else ln1(y))
        h = ln2(a) if pre else a
        z = torch.relu(h @ g(p + "/pwffn/ffn_1/w") + g(p + "/pwffn/ffn_1/b"))
        z = z @ g(p + "/pwffn/ffn_2/w") + g(p + "/pwffn/ffn_2/b")
        return a + f * (z if pre else ln2(z))

    def _chunk(self, feat):
        cfg = self.cfg
        x = self._sub(feat) @ self.g("enc/linear/w") + self.g("enc/linear/b")
        n = x.shape[0]
        x = x + TO.sinusoid_pe(self.seen + n, int(cfg.dmodel), bool(cfg.interleave_relpe), self.dt)[self.seen:]
        for i in range(int(cfg.num_blocks)):
            x = self._block(x, i)
        self.seen += n
        return x

    def feed(self, feat):
        self.pending = torch.cat([self.pending, torch.as_tensor(feat).to(self.dt)], 0)
        out = [torch.zeros(0, int(self.cfg.dmodel), dtype=self.dt)]
        n0 = 4 * self.C
        while self.pending.shape[0] >= n0:
            out.append(self._chunk(self.pending[:n0]))
            self.pending = self.pending[n0:]
        return torch.cat(out, 0)

    def flush(self):
        if self.pending.shape[0] == 0:
            return torch.zeros(0, int(self.cfg.dmodel), dtype=self.dt)
        x, self.pending = self._chunk(self.pending), self.pending[:0]
        return x


def stream_encoder(feat, frames_per_call, W, cfg, dtype=torch.float64):
    """feat [T0, F] of one utterance arriving frames_per_call feature frames at a time -> encoder frames [T', d]"""
    s = EncoderStream(W, cfg, dtype)
    outs = [s.feed(feat[i:i + frames_per_call]) for i in range(0, feat.shape[0], frames_per_call)]
    return torch.cat(outs + [s.flush()], 0)


def offline_alone(feat, W, cfg, **kw):
    """the offline oracle on one utterance alone: feat [T0, F] -> encoder frames [T', d]"""
    enc, lens = TO.encoder(torch.as_tensor(feat)[None], [feat.shape[0]], cfg, W, **kw)
    return enc[0, :lens[0]]
