"""GPU: every kernel of csrc/attn_fused.hip against the float64 restatement of tests/relattn_oracle.py, on every launch branch.

Each kernel is held to the oracle twice, with the bounds derived in that module's docstring (nothing here is fitted to a measured value):
 (a) ALONE, from the oracle's own inputs rounded to their storage types (o, qu, qv, dS bf16; lse, dvec f32), so that a kernel's error is
     its own: tfasr_relattn_bwd_prep (qu, qv bitwise, both planes of dvec, order), tfasr_relattn_fused_bwd_q3 and the merged
     tfasr_relattn_fused_bwd_qk from the oracle's o and lse, tfasr_relattn_fused_bwd_k from the oracle's lse, dvec, qu, qv, and
     tfasr_relattn_dpext from the oracle's bf16 dS and qv against the oracle's dpext OF THOSE VALUES (f32 accumulation only);
 (b) CHAINED as the model runs them: forward, then bwd_q3 + bwd_k + dpext and bwd_prep + bwd_qk + dpext from the forward's own o and lse,
     each route against float64 on its own (route against route: tests/test_attn_bwd_qk_gpu.py).
Cases (relattn_oracle.CASES; dh = 64, ragged lengths) and the branch each is the smallest shape to reach:
 t1            T = 1: 2T = 2 table rows under a 128-row window, every K / V / window row clamped, B*H = 12
 t9            one partial block, H = 3, B*H = 9 (idle workgroups of attn_block_id), negative tile origin in dpext
 t63 t64 t65   one row short of a block, exactly one, one row into the second (ragged last key block)
 h1            one (sample, head): seven idle XCD slots          h8   H = 8
 pad-block     wholly padded query blocks, a partly padded one, shift up to T - 1
 nomask        use_mask = 0, forward and backward: padded rows attend like real ones
 heads36       heads of 36 stored as 64: the padded dims of dq, dk, dv, du, dv_bias, dpext are exactly 0.0; scale = 1/6
 win-16-64     the shipped streaming window                     win-8-inf   unlimited history
 win-5-3       window inside one key block, skipped key blocks, the forward's first processed key block fully masked for some rows
 win-1-0       one visible key per row                          win-wide    STREAM build, window = the utterance: the no-window oracle
 dpext-groups  B = 11, H = 32: tfasr_relattn_dpext with two samples per workgroup group, the last group short, lengths 1, 2 and several < 64
               (tiles skipped by tile_at, negative tile origins)
NOT-WRITTEN ROWS: every output buffer is prefilled with a NaN bit pattern; afterwards the qu / qv / dvec / dS rows of wholly padded 64-query
blocks still hold it and nothing else does.  (The dS columns T .. lds-1 of the written rows ARE written - zeros: the query side stores
whole 8-column chunks below lds, attn_fused.hip:805 - so they are asserted zero there; their consumer masks them all the same, below.)
STALE SCRATCH: NaN planted in exactly the rows (and, for tfasr_relattn_dpext, the columns T .. lds-1) the consumers must not read changes
no bit of dq, dk, dv and leaves du, dv_bias, dpext finite.  du, dv_bias and dpext are f32 atomics whose order differs between two runs, so
the two runs of THOSE are held to twice their f32-sum bound instead of to equality; everywhere they are held to that bound over the oracle.
With TFASR_RELATTN_WRITE_PARITY=1 a full run writes the worst max |gpu - ref| / bound per case and quantity to
profiles/relattn_fused_parity.json."""
import functools
import json
import os

import pytest
import torch

import relattn_oracle as RO
from tensorflowasr_amd import kernels as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF, F32, F64, DH = torch.bfloat16, torch.float32, torch.float64, RO.DH
SENT16, SENT32 = 0x7FA5, 0x7FA5A5A5  # NaN patterns no kernel produces
_PARITY = {}


@pytest.fixture(scope="module", autouse=True)
def parity_profile():
    yield
    if os.environ.get("TFASR_RELATTN_WRITE_PARITY") == "1" and set(RO.CASES) <= set(_PARITY):
        with open(os.path.join(ROOT, "profiles", "relattn_fused_parity.json"), "w") as fh:
            json.dump({"what": "tests/test_relattn_fused_gpu.py: worst max |gpu - ref| / bound per case and quantity (alone/: the kernel from "
                               "the oracle's inputs, q3/ and qk/: chained behind the forward on the two backward routes); bounds as derived "
                               "in tests/relattn_oracle.py", "cases": {k: _PARITY[k] for k in sorted(_PARITY)}}, fh, indent=1)
            fh.write("\n")


@functools.lru_cache(maxsize=2)
def _ref(name):
    x = RO.make_inputs(name)
    f = RO.forward(x["qkv"], x["u"], x["v"], x["pext"], x["lens"], x["B"], x["H"], x["T"], x["scale"], x["use_mask"], x["chunk"], x["hist"])
    fb = RO.forward_bounds(f)
    o16, lse32 = f["out"].to(F32).to(BF), f["lse"].to(F32)
    bk = RO.backward(f, o16, lse32, x["dout"])                          # (a): from the rounded o and lse, as given
    bkc = RO.backward(f, f["out"], f["lse"], x["dout"], o_mag=f["M_out"])  # (b): the exact ones
    return dict(x=x, f=f, fb=fb, o16=o16, lse32=lse32, bk=bk, bb=RO.backward_bounds(f, fb, bk), bkc=bkc, bbc=RO.backward_bounds(f, fb, bkc, chained=True),
                live=RO.live_rows(x["T"], x["lens"], x["use_mask"]))


def _sent(shape, dtype, dev):
    if dtype == BF:
        return torch.full(shape, SENT16, dtype=torch.int16, device=dev).view(BF)
    return torch.full(shape, SENT32, dtype=torch.int32, device=dev).view(F32)


def _is_sent(t):
    return (t.view(torch.int16) == SENT16) if t.dtype == BF else (t.view(torch.int32) == SENT32)


class Run:
    """One case on the device: its inputs and a fresh set of output buffers, sentinel-filled (the atomically accumulated ones zeroed)."""

    def __init__(self, name, dev):
        r = _ref(name)
        x = r["x"]
        self.name, self.r, self.dev = name, r, dev
        self.B, self.H, self.T, self.scale, self.mask = x["B"], x["H"], x["T"], x["scale"], x["use_mask"]
        self.HD, self.lds = self.H * DH, -(-self.T // 8) * 8
        self.win = dict(chunk_size=x["chunk"] or None, history_size=x["hist"])
        self.ck, self.hs = (x["chunk"], x["hist"]) if x["chunk"] else (0, 0)
        self.qkv, self.u, self.v, self.pext, self.dout = (x[k].to(dev) for k in ("qkv", "u", "v", "pext", "dout"))
        self.ln = torch.tensor(x["lens"], dtype=torch.int32, device=dev)
        self.dims = (self.B, self.H, self.T, DH)
        self.bad = []
        self.fresh()

    def fresh(self):
        B, H, T, HD, dev = self.B, self.H, self.T, self.HD, self.dev
        self.dqkv, self.ds = _sent((B * T, 3 * HD), BF, dev), _sent((B, H, T, self.lds), BF, dev)
        self.qu, self.qv, self.dvec = _sent((B * T, HD), BF, dev), _sent((B * T, HD), BF, dev), _sent((2, B, H, T), F32, dev)
        self.du, self.dvb, self.dpext = torch.zeros(HD, device=dev), torch.zeros(HD, device=dev), torch.zeros(2 * T, HD, device=dev)
        return self

    def fwd(self):
        out, lse = _sent((self.B * self.T, self.HD), BF, self.dev), _sent((self.B, self.H, self.T), F32, self.dev)
        K.check(K._L().tfasr_relattn_fused_fwd(K._p(self.qkv), K._p(self.u), K._p(self.v), K._p(self.pext), K._p(self.ln), K._p(out), K._p(lse),
                                               *self.dims, self.scale, int(self.mask), self.ck, self.hs, K._dt(self.qkv), K._stream()), "relattn_fused_fwd")
        return out, lse

    def q3(self, o, lse):
        K.check(K._L().tfasr_relattn_fused_bwd_q3(K._p(self.qkv), K._p(self.u), K._p(self.v), K._p(self.pext), K._p(self.ln), K._p(o), K._p(self.dout),
                                                  K._p(lse), K._p(self.dqkv), self.dqkv.stride(0), K._p(self.du), K._p(self.dvb), K._p(self.ds),
                                                  K._p(self.dvec), K._p(self.dpext), K._p(self.qu), K._p(self.qv), *self.dims, self.lds, self.scale,
                                                  int(self.mask), self.ck, self.hs, K._dt(self.qkv), K._stream()), "relattn_fused_bwd_q3")

    def prep(self, o):
        return K.relattn_bwd_prep(self.qkv, self.u, self.v, self.pext, self.ln, o, self.dout, *self.dims, use_mask=self.mask, qu=self.qu, qv=self.qv,
                                  dvec=self.dvec)[3]

    def qk(self, lse, order, qu=None, qv=None, dvec=None):
        K.relattn_fused_bwd_qk(self.qkv, self.u, self.v, self.pext, self.ln, self.dout, lse, self.qu if qu is None else qu, self.qv if qv is None else qv,
                               self.dvec if dvec is None else dvec, order, self.dqkv, self.du, self.dvb, self.dpext, *self.dims, self.scale,
                               use_mask=self.mask, ds=self.ds, **self.win)

    def bk(self, lse, qu=None, qv=None, dvec=None):
        K.relattn_fused_bwd_k(self.qkv, self.qu if qu is None else qu, self.qv if qv is None else qv, self.pext, self.ln, self.dout, lse,
                              self.dvec if dvec is None else dvec, self.dqkv, *self.dims, self.scale, use_mask=self.mask, **self.win)

    def dpx(self, ds=None, qv=None):
        K.relattn_dpext(self.ds if ds is None else ds, self.qv if qv is None else qv, self.ln, self.dpext, *self.dims, use_mask=self.mask)

    # ---- checks
    def held(self, tag, q, got, ref, bound):
        """max |gpu - ref| / bound <= 1, recorded; where the bound is zero the value is the oracle's exactly"""
        got = got.detach().to("cpu", F64)
        err = (got - ref).abs().nan_to_num(nan=float("inf"))
        ratio = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max()) if err.numel() else 0.0
        rec = _PARITY.setdefault(self.name, {})
        rec[f"{tag}/{q}"] = max(rec.get(f"{tag}/{q}", 0.0), round(ratio, 4))
        print(f"[relattn] {self.name:13s} {tag}/{q:6s} max |gpu - ref| / bound = {ratio:.4f}")
        if not ratio <= 1.0:  # (every quantity of the test is measured and printed before the test fails)
            self.bad.append(f"{tag}/{q}: {ratio}")

    def done(self):
        assert not self.bad, f"{self.name}: " + ", ".join(self.bad)

    def rows(self, live=True):
        m = self.r["live"] if live else ~self.r["live"]
        return m.view(-1).to(self.dev)

    def check_prep_outputs(self, tag, bk, bb, exact_dvec=False):
        """qu / qv bitwise, dvec inside its bound on the written rows; the sentinel on the others and nowhere else"""
        f, live, dead = self.r["f"], self.rows(), self.rows(False)
        for got, want, q in ((self.qu, f["qu"], "qu"), (self.qv, f["qv"], "qv")):
            assert torch.equal(got[live], want.to(BF).to(self.dev)[live]), f"{self.name} {tag}/{q}"
            assert bool(_is_sent(got[dead]).all()) and not bool(_is_sent(got[live]).any()), f"{self.name} {tag}/{q}: written rows"
        lv = self.r["live"][None, :, None, :].expand(2, self.B, self.H, self.T)
        assert bool(_is_sent(self.dvec)[~lv.to(self.dev)].all()) and not bool(_is_sent(self.dvec)[lv.to(self.dev)].any()), f"{self.name} {tag}/dvec: written rows"
        self.held(tag, "dvec", self.dvec.cpu()[lv], bk["dvec"][lv], bb["dvec"][lv])

    def check_query_side(self, tag, bk, bb):
        HD, T = self.HD, self.T
        dq = self.dqkv[:, :HD]
        assert not bool(_is_sent(dq).any()), f"{self.name} {tag}/dq: every row is written"
        self.held(tag, "dq", dq, bk["dq"], bb["dq"])
        lv = self.r["live"][:, None, :].expand(self.B, self.H, T)
        sent = _is_sent(self.ds).cpu()
        assert bool(sent[~lv].all()) and not bool(sent[lv].any()), f"{self.name} {tag}/dS: written rows"
        ds = self.ds.cpu()
        assert float(ds[lv][:, T:].float().abs().max() if self.lds > T else 0.0) == 0.0, f"{self.name} {tag}/dS: columns T .. lds-1"
        self.held(tag, "dS", ds[lv][:, :T], bk["dS"][lv], bb["dS"][lv])
        self.held(tag, "du", self.du, bk["du"], bb["du"])
        self.held(tag, "dvb", self.dvb, bk["dvb"], bb["dvb"])
        self.held(tag, "dpextR", self.dpext[2 * T - 1], bk["dpext"][2 * T - 1], bb["dpext"][2 * T - 1])

    def check_key_side(self, tag, bk, bb):
        HD = self.HD
        assert not bool(_is_sent(self.dqkv[:, HD:]).any()), f"{self.name} {tag}: every dk / dv row is written"
        self.held(tag, "dk", self.dqkv[:, HD:2 * HD], bk["dk"], bb["dk"])
        self.held(tag, "dv", self.dqkv[:, 2 * HD:], bk["dv"], bb["dv"])

    def check_padded_dims(self, tag):
        """heads36: the gradient of a zero-padded head dim is exactly 0.0 (not merely small)"""
        dhl = RO.CASES[self.name].dhl
        if dhl == DH:
            return
        pad = (torch.arange(DH) >= dhl).repeat(self.H).to(self.dev)
        for q, t in (("dq dk dv", self.dqkv[:, pad.repeat(3)]), ("du", self.du[pad]), ("dvb", self.dvb[pad]), ("dpext", self.dpext[:, pad])):
            assert bool((t.float() == 0).all()), f"{self.name} {tag}/{q}: padded head dims"


def _order(lens, T):
    return sorted(range(len(lens)), key=lambda s: (-min(lens[s], T), s))


def _to(t, dev, dtype):
    return t.to(dtype).to(dev).contiguous()


# ------------------------------------------------------------------------------------ (a) alone
@pytest.mark.parametrize("name", list(RO.CASES))
def test_forward(dev, name):
    g = Run(name, dev)
    out, lse = g.fwd()
    torch.cuda.synchronize()
    assert not bool(_is_sent(out).any()) and not bool(_is_sent(lse).any()), "every row of out and lse is written"
    g.held("alone", "out", out, g.r["f"]["out"], g.r["fb"]["out"])
    g.held("alone", "lse", lse, g.r["f"]["lse"], g.r["fb"]["lse"])
    g.done()


@pytest.mark.parametrize("name", list(RO.CASES))
def test_backward_kernels_alone(dev, name):
    g = Run(name, dev)
    r, bk, bb = g.r, g.r["bk"], g.r["bb"]
    o, lse = r["o16"].to(dev), r["lse32"].to(dev)
    # preparation
    order = g.prep(o)
    torch.cuda.synchronize()
    assert order.cpu().tolist() == _order(r["x"]["lens"], g.T)
    g.check_prep_outputs("alone-prep", bk, bb)
    # query side, two-launch route
    g.fresh().q3(o, lse)
    torch.cuda.synchronize()
    g.check_prep_outputs("alone-q3", bk, bb)
    g.check_query_side("alone-q3", bk, bb)
    assert bool(_is_sent(g.dqkv[:, g.HD:]).all()), "the query side writes no dk / dv"
    assert float(g.dpext[:2 * g.T - 1].abs().max()) == 0.0, "the query side writes the bias row of dpext only"
    # key side, from the oracle's lse, dvec, qu, qv (rows of wholly padded blocks: the sentinel NaN, as an executor's scratch may hold)
    dead = g.rows(False)
    qu, qv = _to(r["f"]["qu"], dev, BF), _to(r["f"]["qv"], dev, BF)
    dvec = _to(bk["dvec"], dev, F32)
    qu[dead], qv[dead] = float("nan"), float("nan")
    dvec.view(2, g.B, g.H, g.T)[:, (~r["live"]).to(dev)[:, None, :].expand(g.B, g.H, g.T)] = float("nan")
    g.fresh().bk(lse, qu, qv, dvec)
    torch.cuda.synchronize()
    g.check_key_side("alone-k", bk, bb)
    assert bool(_is_sent(g.dqkv[:, :g.HD]).all()), "the key side writes no dq"
    # merged launch from the same
    g.fresh().qk(lse, torch.tensor(_order(r["x"]["lens"], g.T), dtype=torch.int32, device=dev), qu, qv, dvec)
    torch.cuda.synchronize()
    g.check_query_side("alone-qk", bk, bb)
    g.check_key_side("alone-qk", bk, bb)
    g.check_padded_dims("alone-qk")
    # table gradient from the oracle's bf16 dS (NaN in the rows of wholly padded blocks and in the columns T .. lds-1) and qv
    ds = torch.full((g.B, g.H, g.T, g.lds), float("nan"), dtype=BF)
    lv = r["live"][:, None, :].expand(g.B, g.H, g.T)
    ds[..., :g.T][lv] = bk["dS"].to(F32).to(BF)[lv]
    want = RO.dpext_of(r["f"], ds[..., :g.T].masked_fill(~lv[..., None], 0.0))
    g.fresh().dpx(ds.to(dev), qv)
    torch.cuda.synchronize()
    g.held("alone", "dpext", g.dpext, want["dpext"], want["B_dpext"])
    g.done()


# ------------------------------------------------------------------------------------ (b) chained
@pytest.mark.parametrize("route", ["q3", "qk"])
@pytest.mark.parametrize("name", list(RO.CASES))
def test_chained_backward_route(dev, name, route):
    g = Run(name, dev)
    bk, bb = g.r["bkc"], g.r["bbc"]
    o, lse = g.fwd()
    if route == "q3":
        g.q3(o, lse)
        g.bk(lse)
    else:
        g.qk(lse, g.prep(o))
    g.dpx()
    torch.cuda.synchronize()
    HD, T = g.HD, g.T
    assert not bool(_is_sent(g.dqkv).any()), "every row of dq, dk, dv is written"
    g.held(route, "dq", g.dqkv[:, :HD], bk["dq"], bb["dq"])
    g.check_key_side(route, bk, bb)
    lv = g.r["live"][:, None, :].expand(g.B, g.H, T)
    g.held(route, "dS", g.ds.cpu()[lv][:, :T], bk["dS"][lv], bb["dS"][lv])
    g.held(route, "du", g.du, bk["du"], bb["du"])
    g.held(route, "dvb", g.dvb, bk["dvb"], bb["dvb"])
    g.held(route, "dpext", g.dpext, bk["dpext"], bb["dpext"])
    g.check_padded_dims(route)
    g.done()


# ------------------------------------------------------------------------------------ stale scratch
def _two_runs(g, launch):
    """`launch(fill)` with NaN / zeros planted; -> the outputs of both"""
    outs = []
    for fill in (float("nan"), 0.0):
        g.fresh()
        launch(fill)
        torch.cuda.synchronize()
        outs.append((g.dqkv.clone(), g.du.clone(), g.dvb.clone(), g.dpext.clone()))
    return outs


def _same_atomics(g, a, b, M, what):
    a, b = a.cpu().to(F64), b.cpu().to(F64)
    assert bool(torch.isfinite(a).all()), what
    assert bool(((a - b).abs() <= 2 * (g.B * g.T + g.T + 4) * RO.U32 * M).all()), what


@pytest.mark.parametrize("kernel", ["bwd_k", "bwd_qk"])
def test_stale_scratch_rows_stay_out_of_the_gradients(dev, kernel):
    g = Run("pad-block", dev)
    r, bk = g.r, g.r["bk"]
    lse = r["lse32"].to(dev)
    dead = g.rows(False)
    assert bool(dead.any())
    order = torch.tensor(_order(r["x"]["lens"], g.T), dtype=torch.int32, device=dev)

    def launch(fill):
        qu, qv, dvec = _to(r["f"]["qu"], dev, BF), _to(r["f"]["qv"], dev, BF), _to(bk["dvec"], dev, F32)
        qu[dead], qv[dead] = fill, fill
        dvec.view(2, g.B, g.H, g.T)[:, (~r["live"]).to(dev)[:, None, :].expand(g.B, g.H, g.T)] = fill
        g.ds.fill_(fill)
        g.bk(lse, qu, qv, dvec) if kernel == "bwd_k" else g.qk(lse, order, qu, qv, dvec)

    (a, au, av, ap), (b, bu, bv, bp) = _two_runs(g, launch)
    cols = slice(g.HD, None) if kernel == "bwd_k" else slice(None)
    assert bool(torch.isfinite(a[:, cols].float()).all()) and torch.equal(a[:, cols].view(torch.int16), b[:, cols].view(torch.int16))
    if kernel == "bwd_qk":
        _same_atomics(g, au, bu, bk["M_du"], "du")
        _same_atomics(g, av, bv, bk["M_dvb"], "dv bias")
        _same_atomics(g, ap, bp, bk["M_dpext"], "dpext bias row")


def test_stale_scratch_stays_out_of_the_table_gradient(dev):
    g = Run("heads36", dev)  # T = 150, lds = 152: two columns past T
    r, bk = g.r, g.r["bk"]
    assert g.lds > g.T
    lv = r["live"][:, None, :].expand(g.B, g.H, g.T)
    qv0 = _to(r["f"]["qv"], dev, BF)
    dead = g.rows(False)

    def launch(fill):
        ds = torch.full((g.B, g.H, g.T, g.lds), fill, dtype=BF)
        ds[..., :g.T][lv] = bk["dS"].to(F32).to(BF)[lv]
        qv = qv0.clone()
        qv[dead] = fill
        g.dpx(ds.to(dev), qv)

    (_, _, _, ap), (_, _, _, bp) = _two_runs(g, launch)
    _same_atomics(g, ap, bp, bk["M_dpext"], "dpext")
    assert float(ap.abs().max()) > 0
