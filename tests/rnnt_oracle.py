"""float64 NumPy oracle of the RNN-Transducer encoder (tensorflowasr_amd/rnnt.py), offline and chunked, written from the reference's
layers:

    models/encoders/rnnt.py:73-85      RnnTransducerBlock.call   [TimeReduction] -> LSTM -> [LayerNormalization] -> Dense -> [TimeReduction]
    models/encoders/rnnt.py:92-121     RnnTransducerBlock.call_next (the LSTM continued from given states)
    models/layers/subsampling.py:34-40 TimeReduction.call        zero-pad T to a multiple of f, [B, T, d] -> [B, T / f, f d], ceil(len / f)
    keras LSTM(zero_output_for_mask)   gates i, f, c, o; a masked step carries the state and emits zeros

W maps the ParamStore names (enc/block_i/lstm/{k,rk,b}, enc/block_i/ln/{g,b}, enc/block_i/projection/{w,b}) to arrays.  `rnd` rounds what
a bf16 device pipeline stores (features, LSTM input projections, h, LayerNorm output, block output) and `wrnd` the kernels: the rounding
floor the bf16 test compares against.

encoder()      the offline walk of a (padded) batch, every row computed as the reference computes it - padded rows included
call_next()    the reference's call_next over one chunk, including its mask rule for a `pre` block (the LSTM is handed the mask of the
               block's un-reduced INPUT, of which a recurrence over T / f steps reads the first T / f columns)
StreamWalk     one utterance fed in pieces: leftover rows in front of every reduction are carried, the last group is zero-padded at the
               end - the frames of the utterance run alone, whatever the pieces"""
import numpy as np

LN_EPS = 1e-3


def _id(x):
    return x


def bf16_round(x):
    """round-to-nearest-even to bfloat16, kept in float64"""
    a = np.ascontiguousarray(np.asarray(x, np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(a.shape).astype(np.float64)


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def modules(cfg):
    from tensorflowasr_amd.params import rnnt_modules

    return rnnt_modules(cfg)


def _w(W, name, dtype, wrnd=_id):
    return wrnd(np.asarray(W[name], np.float64)).astype(dtype)


def lstm(x, mask, k, rk, b, h0=None, c0=None, rnd=_id):
    """x [B, T, Din], mask [B, >= T] bool -> (y [B, T, P] zeros where masked, h, c)"""
    B, T, _ = x.shape
    P = rk.shape[0]
    h = np.zeros((B, P), x.dtype) if h0 is None else np.asarray(h0, x.dtype)
    c = np.zeros((B, P), x.dtype) if c0 is None else np.asarray(c0, x.dtype)
    xg = rnd(x @ k + b).astype(x.dtype)
    y = np.zeros((B, T, P), x.dtype)
    for t in range(T):
        z = xg[:, t] + h @ rk
        i, f, g, o = _sig(z[:, :P]), _sig(z[:, P:2 * P]), np.tanh(z[:, 2 * P:3 * P]), _sig(z[:, 3 * P:])
        cn = f * c + i * g
        hn = rnd(o * np.tanh(cn)).astype(x.dtype)
        m = mask[:, t, None]
        y[:, t] = np.where(m, hn, 0.0)
        h, c = np.where(m, hn, h), np.where(m, cn, c)
    return y, h, c


def layer_norm(x, g, b):
    m = x.mean(-1, keepdims=True)
    v = ((x - m) ** 2).mean(-1, keepdims=True)
    return (x - m) / np.sqrt(v + x.dtype.type(LN_EPS)) * g + b


def time_reduction(x, lens, f):
    B, T, d = x.shape
    Tp = -(-T // f) * f
    x = np.concatenate([x, np.zeros((B, Tp - T, d), x.dtype)], 1)
    return x.reshape(B, Tp // f, f * d), [-(-n // f) for n in lens]


def seq_mask(lens, T):
    return np.arange(T)[None, :] < np.asarray(lens)[:, None]


def tail(y, m, W, dtype, rnd=_id, wrnd=_id):
    p = m["name"]
    if m["ln"]:
        y = rnd(layer_norm(y, _w(W, p + "/ln/g", dtype), _w(W, p + "/ln/b", dtype))).astype(dtype)
    return rnd(y @ _w(W, p + "/projection/w", dtype, wrnd) + _w(W, p + "/projection/b", dtype)).astype(dtype)


def block(x, lens, m, W, dtype=np.float64, state=None, rnd=_id, wrnd=_id, lstm_mask=None):
    """one RnnTransducerBlock -> (out, lengths, (h, c)); lstm_mask overrides the mask the LSTM sees (call_next's rule)"""
    p, f = m["name"], m["factor"]
    if m["position"] == "pre" and f > 1:
        x, lens = time_reduction(x, lens, f)
    T = x.shape[1]
    mask = seq_mask(lens, T) if lstm_mask is None else np.asarray(lstm_mask)[:, :T]
    h0, c0 = (None, None) if state is None else state
    y, h, c = lstm(x, mask, _w(W, p + "/lstm/k", dtype, wrnd), _w(W, p + "/lstm/rk", dtype, wrnd), _w(W, p + "/lstm/b", dtype), h0, c0, rnd)
    out = tail(y, m, W, dtype, rnd, wrnd)
    if m["position"] == "post" and f > 1:
        out, lens = time_reduction(out, lens, f)
    return out, lens, (h, c)


def encoder(feats, flen, cfg, W, dtype=np.float64, rnd=_id, wrnd=_id, trace=None):
    """RnnTransducerEncoder.call on features [B, T, F] (the Reshape's output) -> (enc [B, T', cfg.dmodel], lengths, states [B, L, 2, P]).
    Every LSTM sees sequence_mask(its block's lengths): block 0's is the mask FeatureExtraction attaches to the features
    (feature_extraction.py:315-322), which the Reshape and the layers behind it pass on."""
    x, lens = rnd(np.asarray(feats, np.float64)).astype(dtype), [int(n) for n in flen]
    states = []
    for m in modules(cfg):
        if trace is not None:
            trace[m["name"]] = (x.copy(), list(lens))
        x, lens, (h, c) = block(x, lens, m, W, dtype, None, rnd, wrnd)
        states.append(np.stack([h, c], 1))
    return x, lens, np.stack(states, 1)


def call_next(feats, flen, states, cfg, W, dtype=np.float64):
    """RnnTransducerEncoder.call_next (encoders/rnnt.py:188-211) over one chunk: states [B, L, 2, P] -> (out, lengths, new states).
    Each block hands its LSTM `mask=backend.get_keras_mask(inputs)` - the mask of the block's INPUT (:104-109).  For a `pre` block with
    a reduction that mask still has the un-reduced length, and the recurrence over T / f steps reads its first T / f columns."""
    x, lens = np.asarray(feats, np.float64).astype(dtype), [int(n) for n in flen]
    new = []
    for i, m in enumerate(modules(cfg)):
        in_mask = seq_mask(lens, x.shape[1])
        st = (states[:, i, 0], states[:, i, 1])
        x, lens, (h, c) = block(x, lens, m, W, dtype, st, lstm_mask=in_mask)
        new.append(np.stack([h, c], 1))
    return x, lens, np.stack(new, 1)


def boundary_factors(cfg):
    """The reductions as the chunked walks apply them, one per block boundary: [pre_0, post_0 * pre_1, ..., post_{L-1}].  A `post` reduction
    by f followed by a `pre` reduction by g groups f g consecutive rows (zero rows pad either), and no layer sits between them."""
    mods = modules(cfg)
    pre = [m["factor"] if m["position"] == "pre" else 1 for m in mods]
    post = [m["factor"] if m["position"] == "post" else 1 for m in mods]
    return [pre[0]] + [post[i] * pre[i + 1] for i in range(len(mods) - 1)] + [post[-1]]


class StreamWalk:
    """one utterance in pieces: step(rows [n, F], final) -> the encoder frames that became complete"""

    def __init__(self, cfg, W, dtype=np.float64, rnd=_id, wrnd=_id):
        self.cfg, self.W, self.dtype, self.rnd, self.wrnd = cfg, W, dtype, rnd, wrnd
        self.mods, self.fb = modules(cfg), boundary_factors(cfg)
        self.carry = [None] * len(self.fb)
        self.hc = [None] * len(self.mods)

    def _reduce(self, i, rows, final):
        f = self.fb[i]
        buf = rows if self.carry[i] is None else np.concatenate([self.carry[i], rows], 0)
        if final and buf.shape[0] % f:
            buf = np.concatenate([buf, np.zeros((f - buf.shape[0] % f, buf.shape[1]), buf.dtype)], 0)
        g = buf.shape[0] // f
        self.carry[i] = buf[g * f:]
        return buf[:g * f].reshape(g, f * buf.shape[1])

    def step(self, rows, final=False):
        x = self.rnd(np.asarray(rows, np.float64)).astype(self.dtype)
        for i, m in enumerate(self.mods):
            x = self._reduce(i, x, final)
            p = m["name"]
            h0, c0 = (None, None) if self.hc[i] is None else self.hc[i]
            y, h, c = lstm(x[None], np.ones((1, x.shape[0]), bool), _w(self.W, p + "/lstm/k", self.dtype, self.wrnd),
                           _w(self.W, p + "/lstm/rk", self.dtype, self.wrnd), _w(self.W, p + "/lstm/b", self.dtype), h0, c0, self.rnd)
            self.hc[i] = (h, c)
            x = tail(y[0], m, self.W, self.dtype, self.rnd, self.wrnd)
        return self._reduce(len(self.mods), x, final)

    def states(self):
        """[L, 2, P]: (h, c) per block"""
        return np.stack([np.stack([h[0], c[0]]) for h, c in self.hc])
