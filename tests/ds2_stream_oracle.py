"""float64 restatements for the DeepSpeech2 streaming tests: the LSTM recurrence of tests/ds2_oracle.py continued from an initial state,
and the unidirectional encoder run chunk by chunk with everything a stream carries - the conv blocks' input tails, the LSTM states and
the RowConv1D tails.  Everything here runs on the CPU."""
import numpy as np
import torch
import torch.nn.functional as F

import ds2_oracle as DO


def lstm_state(xg, rk, lengths, h0=None, c0=None, hround=None):
    """DO.lstm (one forward direction) from the state (h0, c0) [B, P] instead of zeros -> (y [B, T, P], h_last, c_last); a step
    t >= lengths[b] carries the state and emits zeros.  hround: rounding of the carried h, the incoming h0 included."""
    xg, rk = torch.as_tensor(xg).double(), torch.as_tensor(rk).double()
    B, T, P4 = xg.shape
    P = P4 // 4
    h = torch.zeros(B, P, dtype=torch.float64) if h0 is None else torch.as_tensor(h0).double()
    c = torch.zeros(B, P, dtype=torch.float64) if c0 is None else torch.as_tensor(c0).double()
    if hround is not None:
        h = hround(h)
    y = torch.zeros(B, T, P, dtype=torch.float64)
    lengths = torch.as_tensor(np.asarray(lengths)).long()
    for t in range(T):
        z = xg[:, t] + h @ rk
        i, f, g, o = torch.sigmoid(z[:, :P]), torch.sigmoid(z[:, P:2 * P]), torch.tanh(z[:, 2 * P:3 * P]), torch.sigmoid(z[:, 3 * P:])
        cn = f * c + i * g
        hn = o * torch.tanh(cn)
        m = (t < lengths)[:, None]
        y[:, t] = torch.where(m, hn, torch.zeros_like(hn))
        if hround is not None:
            hn = hround(hn)
        h, c = torch.where(m, hn, h), torch.where(m, cn, c)
    return y, h, c


class ChunkedEncoder:
    """One utterance of the unidirectional encoder (DO.encoder with conv_padding "causal", forward LSTMs, RowConv1D) fed in pieces of
    feature frames.  Carried: per conv block the last kh - 1 rows of its input (zeros at the start = the causal padding), per RnnBlock
    (h, c) and the last K - 1 rows of the LSTM's output.  A piece that is not the utterance's last must be a multiple of the time
    reduction factor long."""

    def __init__(self, cfg, W):
        assert cfg.conv_padding == "causal" and not cfg.rnn_bidirectional
        self.cfg, self.W = cfg, W
        self.convs, self.rnns, self.fcs = DO.topology(cfg)
        self.conv_tails = [None] * len(self.convs)
        P = int(cfg.rnn_units)
        self.hc = [(torch.zeros(1, P, dtype=torch.float64), torch.zeros(1, P, dtype=torch.float64)) for _ in self.rnns]
        self.row_tails = [None] * len(self.rnns)

    def states(self):
        """[1, nlayers, 2, P]: the reference's layout (encoders/deepspeech2.py:330-337), states ordered (h, c)"""
        return torch.stack([torch.stack([h, c], 1) for h, c in self.hc], 1)

    def step(self, feats):
        """feats [n, F] -> [ceil-reduced n, dmodel]"""
        cfg, W = self.cfg, self.W
        x = torch.as_tensor(feats).double()[None, :, :, None]
        for i, m in enumerate(self.convs):
            w = W[m["name"] + "/conv2d/w"].double()
            kh, kw = w.shape[:2]
            st, sf = m["strides"]
            if self.conv_tails[i] is None:
                self.conv_tails[i] = torch.zeros(1, kh - 1, x.shape[2], x.shape[3], dtype=torch.float64)
            win = torch.cat([self.conv_tails[i], x], 1)
            self.conv_tails[i] = win[:, win.shape[1] - (kh - 1):]
            # time: "valid" over tail ++ rows; frequency: the causal padding
            xp = F.pad(win.permute(0, 3, 1, 2), (kw - 1, 0, 0, 0))
            y = F.conv2d(xp, w.permute(3, 2, 0, 1).contiguous(), stride=(st, sf)).permute(0, 2, 3, 1)
            assert y.shape[1] == -(-x.shape[1] // st)
            x = torch.relu(DO.batchnorm(y + W[m["name"] + "/conv2d/b"].double(), W, m["name"] + "/bn"))
        T = x.shape[1]
        x = x.reshape(1, T, -1)
        for i, r in enumerate(self.rnns):
            name = r["dirs"][0]
            xg = x @ W[name + "/k"].double() + W[name + "/b"].double()
            y, h, c = lstm_state(xg, W[name + "/rk"], [T], *self.hc[i])
            self.hc[i] = (h, c)
            if r["rowconv"]:
                w = W[r["rowconv"] + "/conv/w"].double()
                K = w.shape[0]
                if self.row_tails[i] is None:
                    self.row_tails[i] = torch.zeros(1, K - 1, y.shape[2], dtype=torch.float64)
                win = torch.cat([self.row_tails[i], y], 1)
                self.row_tails[i] = win[:, win.shape[1] - (K - 1):]
                conv = F.conv1d(win.transpose(1, 2), w.t().reshape(-1, 1, K).contiguous(), groups=y.shape[2]).transpose(1, 2)
                y = torch.relu(DO.batchnorm(conv, W, r["rowconv"] + "/bn"))
            x = y
        for name in self.fcs:
            x = torch.relu(x @ W[name + "/fc/w"].double() + W[name + "/fc/b"].double())
        return x[0]
