"""CPU: tests/relattn_oracle.py is the attention of the reference, its bounds admit a correct kernel and reject a subtly wrong one.

 pin       the oracle's forward and every gradient against torch autograd in float64 on oracle/conformer_ref.py::rel_attention_core - the
           reference's own formulation (rel_left_shift, the per-sample rolled / zeroed position encoding behind the projection = table rows
           shift .. shift + 2 len - 2 and the bias row, compute_streaming_mask, the auto mask), not the gather identity - at every case of
           relattn_oracle.CASES with T <= 130.  q + u / q + v enter as the oracle's rounded values (the one stated difference; -1e9 against
           exactly zero outside the window is none in float64): agreement below 1e-12 of the largest element.
 admits    a torch-f32 emulation with the kernels' rounding points - bf16 P over an f32 row sum, bf16 out, bf16 dS, bf16 P^T, bf16 gradient
           stores - chained as the model runs it (backward from its own o and lse) lies inside every bound at every case.
 rejects   the emulation with ONE index fault exceeds a bound at the case named beside it (input scales: relattn_oracle.CASES)."""
import functools
import math

import pytest
import torch

import relattn_oracle as RO
from oracle import conformer_ref as R

F32, F64, BF, DH = torch.float32, torch.float64, torch.bfloat16, RO.DH
QUANT = ("out", "lse", "dS", "dq", "dk", "dv", "du", "dvb", "dpext")


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """forward, its bounds, the chained backward (from the oracle's exact o and lse, M_dS over M_out) and its bounds - computed once"""
    x = RO.make_inputs(name)
    f = RO.forward(x["qkv"], x["u"], x["v"], x["pext"], x["lens"], x["B"], x["H"], x["T"], x["scale"], x["use_mask"], x["chunk"], x["hist"])
    fb = RO.forward_bounds(f)
    bk = RO.backward(f, f["out"], f["lse"], x["dout"], o_mag=f["M_out"])
    return x, f, fb, bk, RO.backward_bounds(f, fb, bk, chained=True)


# ------------------------------------------------------------------------------------ pin
@pytest.mark.parametrize("name", [n for n, c in RO.CASES.items() if c.T <= 130])
def test_oracle_is_the_reference_attention(name):
    x, f, _, _, _ = _oracle(name)
    c = RO.CASES[name]
    B, H, T = c.B, c.H, c.T
    bk = RO.backward(f, f["out"], f["lse"], x["dout"])
    qu = f["qu"].view(B, T, H, DH).clone().requires_grad_(True)
    qv = f["qv"].view(B, T, H, DH).clone().requires_grad_(True)
    kv = x["qkv"].to(F64).view(B, T, 3, H, DH)
    k, vv = kv[:, :, 1].clone().requires_grad_(True), kv[:, :, 2].clone().requires_grad_(True)
    pe = x["pext"].to(F64).view(2 * T, H, DH).clone().requires_grad_(True)
    # what the projection of the rolled, zeroed encoding is: table rows shift .. shift + 2 len - 2, then the projection's bias
    rows = []
    for n in c.lens:
        r = torch.arange(2 * T - 1)
        rows.append(torch.where(r < 2 * n - 1, r + T - n, torch.full_like(r, 2 * T - 1)))
    p = pe[torch.stack(rows)]  # [B, 2T-1, H, dh]
    win = dict(chunk_size=c.chunk, history_size=c.hist) if c.chunk else {}
    ctx, probs = R.rel_attention_core(torch.zeros_like(qu), k, vv, p, qu, qv, c.dhl, list(c.lens), c.use_mask, **win)
    ctx.backward(x["dout"].to(F64).view(B, T, H, DH))

    def same(a, b, what):
        a, b = a.detach(), b.detach()
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), what

    same(f["_p"], probs, "probabilities")
    same(f["out"], ctx.detach().reshape(B * T, H * DH), "out")
    same(torch.exp(f["_sm"] - f["lse"][..., None]).sum(-1), torch.ones(B, H, T, dtype=F64), "lse")
    same(bk["dq"], (qu.grad + qv.grad).reshape(B * T, H * DH), "dq")
    same(bk["dk"], k.grad.reshape(B * T, H * DH), "dk")
    same(bk["dv"], vv.grad.reshape(B * T, H * DH), "dv")
    same(bk["du"], qu.grad.sum((0, 1)).reshape(-1), "du")
    same(bk["dvb"], qv.grad.sum((0, 1)).reshape(-1), "dv bias")
    same(bk["dpext"], pe.grad.reshape(2 * T, H * DH), "dpext")
    # dS and dvec are not autograd quantities of the reference: dS through the score gradient it implies, D and the bias score by definition
    o, do = f["out"].view(B, T, H, DH), x["dout"].to(F64).view(B, T, H, DH)
    same(bk["dvec"][0], (o * do).sum(-1).permute(0, 2, 1), "D")
    same(bk["dvec"][1], torch.einsum("bthd,hd->bht", qv.detach(), pe.detach()[2 * T - 1]), "bias-row score")
    assert float((bk["dS"] * (f["_idx"] == 2 * T - 1)[:, None]).abs().max()) == 0.0
    same(RO.dpext_of(f, bk["dS"])["dpext"][:2 * T - 1], bk["dpext"][:2 * T - 1], "dpext from the unskewed dS")


def test_window_as_wide_as_the_utterance_is_no_window():
    x, f, _, _, _ = _oracle("win-wide")
    g = RO.forward(x["qkv"], x["u"], x["v"], x["pext"], x["lens"], x["B"], x["H"], x["T"], x["scale"], x["use_mask"], 0, 0)
    assert torch.equal(f["out"], g["out"]) and torch.equal(f["lse"], g["lse"])


# ------------------------------------------------------------------------------------ emulation
def _index(T, lens, dr=0, dthr=0, bias_at=None):
    """relattn_oracle.pair_index with a fault: skew off by dr, validity threshold off by dthr, the bias row read at table row `bias_at`"""
    ln = torch.tensor(lens).clamp(max=T)[:, None, None]
    r = (T - 1 - torch.arange(T)[:, None] + torch.arange(T)[None, :])[None] + dr
    idx = torch.where(r < 2 * ln - 1 + dthr, (r + T - ln).clamp(0, 2 * T - 1), torch.full_like(r, 2 * T - 1))
    return idx if bias_at is None else torch.where(idx == bias_at, torch.full_like(idx, 2 * T - 1), idx)


def emulate(x, idx=None, vis=None, padded=None, dpext_skip=()):
    """The kernels' arithmetic in torch f32 with their rounding points, forward then backward from its own o and lse.
    dpext_skip: samples left out of the table gradient's rows 0 .. 2T-2."""
    B, H, T, scale = x["B"], x["H"], x["T"], x["scale"]
    q3 = x["qkv"].to(F32).view(B, T, 3, H, DH)
    qu = (q3[:, :, 0] + x["u"].view(H, DH)).to(BF).to(F32).permute(0, 2, 1, 3)
    qv = (q3[:, :, 0] + x["v"].view(H, DH)).to(BF).to(F32).permute(0, 2, 1, 3)
    k, vv = q3[:, :, 1].permute(0, 2, 1, 3), q3[:, :, 2].permute(0, 2, 1, 3)
    pe = x["pext"].to(F32).view(2 * T, H, DH).permute(1, 0, 2)
    do = x["dout"].to(F32).view(B, T, H, DH).permute(0, 2, 1, 3)
    idx = RO.pair_index(T, x["lens"]) if idx is None else idx
    padded = RO.padded_rows(T, x["lens"], x["use_mask"]) if padded is None else padded
    vis = RO.visible(T, *RO.window(T, x["chunk"], x["hist"]), padded) if vis is None else vis
    idxe, pm, vm = idx[:, None].expand(B, H, T, T), padded[:, None, :, None], ~vis[:, None]
    t = ((qu @ k.transpose(2, 3) + torch.gather(torch.einsum("bhid,hcd->bhic", qv, pe), 3, idxe)) * F32_(scale)).masked_fill(pm, 0.0)
    m = t.masked_fill(vm, -math.inf).amax(-1, keepdim=True)
    pu = torch.exp(t - m).masked_fill(vm, 0.0)
    l = pu.sum(-1, keepdim=True)                                        # the row sum: unrounded f32 values
    o = ((pu.to(BF).to(F32) @ vv) / l).to(BF)                           # bf16 P for P V, bf16 out
    lse = (m + torch.log(l))[..., 0]
    of = o.to(F32)
    p = torch.exp(t - lse[..., None]).masked_fill(vm, 0.0)
    D = (do * of).sum(-1, keepdim=True)
    dS = (p * ((do @ vv.transpose(2, 3)) * F32_(scale) - D * F32_(scale))).masked_fill(pm, 0.0)
    dSb = dS.to(BF).to(F32)                                             # bf16 dS for every product
    table = (idxe != 2 * T - 1)
    G = torch.zeros(B, H, T, 2 * T).scatter_add_(3, idxe, dSb * table)
    bsum = (dS * ~table).sum(-1)                                        # the bias row's share: summed unrounded
    dqu = dSb @ k
    dqv = torch.einsum("bhic,hcd->bhid", G, pe) + bsum[..., None] * pe[:, None, 2 * T - 1]
    keep = torch.tensor([b not in dpext_skip for b in range(B)], dtype=F32)[:, None, None, None]
    dpext = torch.einsum("bhic,bhid->chd", G * keep, qv)
    dpext[2 * T - 1] = torch.einsum("bhi,bhid->hd", bsum, qv)
    rows = RO._rows
    return dict(out=rows(of), lse=lse, dS=dSb * table, dq=rows((dqu + dqv).to(BF).to(F32)), dk=rows((dSb.transpose(2, 3) @ qu).to(BF).to(F32)),
                dv=rows((p.to(BF).to(F32).transpose(2, 3) @ do).to(BF).to(F32)), du=dqu.sum((0, 2)).reshape(-1), dvb=dqv.sum((0, 2)).reshape(-1),
                dpext=dpext.reshape(2 * T, H * DH))


def F32_(v):
    return torch.tensor(v, dtype=F32)


def _ratios(name, e):
    """max |emulation - oracle| / bound per quantity (0 / 0 = 0: where the bound is zero the value must be the oracle's)"""
    _, f, fb, bk, bb = _oracle(name)
    out = {}
    for q in QUANT:
        ref, bound = (f[q], fb[q]) if q in ("out", "lse") else (bk[q], bb[q])
        err = (e[q].to(F64) - ref).abs()
        out[q] = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    return out


@pytest.mark.parametrize("name", list(RO.CASES))
def test_bounds_admit_the_emulated_kernel(name):
    x = _oracle(name)[0]
    rat = _ratios(name, emulate(x))
    print(f"\n[relattn oracle] {name}: " + " ".join(f"{q} {v:.3f}" for q, v in rat.items()))
    assert max(rat.values()) <= 1.0, rat


def _win(x, dlo=0, dhi=0):
    T = x["T"]
    lo, hi = RO.window(T, x["chunk"], x["hist"])
    return RO.visible(T, (lo + dlo).clamp(0, T), (hi + dhi).clamp(0, T), RO.padded_rows(T, x["lens"], x["use_mask"]))


def _drop_key(x, j):
    vis = _win(x).clone()
    vis[:, :, j] &= RO.padded_rows(x["T"], x["lens"], x["use_mask"])  # (padded rows keep their uniform attention)
    return vis


def _last_of_groups(x):
    n = RO.dpext_bchunk(x["B"], x["H"], x["T"])
    assert n > 1
    return tuple(b for b in range(x["B"]) if b % n == n - 1)


MUTANTS = [
    # fault, the case that exercises it, emulate() arguments from the case's inputs
    ("skew+1", "h8", lambda x: dict(idx=_index(x["T"], x["lens"], dr=1))),
    ("skew-1", "pad-block", lambda x: dict(idx=_index(x["T"], x["lens"], dr=-1))),
    ("threshold+1", "h8", lambda x: dict(idx=_index(x["T"], x["lens"], dthr=1))),
    ("threshold-1", "pad-block", lambda x: dict(idx=_index(x["T"], x["lens"], dthr=-1))),
    ("key-64-dropped", "t65", lambda x: dict(vis=_drop_key(x, 64))),
    ("key-63-dropped", "h8", lambda x: dict(vis=_drop_key(x, 63))),
    ("lo+1", "win-16-64", lambda x: dict(vis=_win(x, dlo=1))),
    ("lo-1", "win-5-3", lambda x: dict(vis=_win(x, dlo=-1))),
    ("hi+1", "win-5-3", lambda x: dict(vis=_win(x, dhi=1))),
    ("hi-1", "win-16-64", lambda x: dict(vis=_win(x, dhi=-1))),
    ("bias-row-for-table-row", "h8", lambda x: dict(idx=_index(x["T"], x["lens"], bias_at=x["T"] - 1))),
    ("padded-row-as-real", "t9", lambda x: dict(padded=torch.zeros(x["B"], x["T"], dtype=torch.bool), vis=_win(dict(x, use_mask=False)))),
    ("padded-row-as-real", "pad-block", lambda x: dict(padded=torch.zeros(x["B"], x["T"], dtype=torch.bool), vis=_win(dict(x, use_mask=False)))),
    ("dpext-last-of-group", "dpext-groups", lambda x: dict(dpext_skip=_last_of_groups(x))),
]


@pytest.mark.parametrize("fault,name,args", MUTANTS, ids=[f"{m[0]}@{m[1]}" for m in MUTANTS])
def test_bounds_reject_one_index_fault(fault, name, args):
    x = _oracle(name)[0]
    rat = _ratios(name, emulate(x, **args(x)))
    print(f"\n[relattn oracle] {fault} at {name}: " + " ".join(f"{q} {v:.3g}" for q, v in rat.items()))
    touched = ("dpext",) if fault == "dpext-last-of-group" else QUANT
    assert max(rat[q] for q in touched) > 1.0, rat


def test_cases_reach_the_branches_they_are_listed_for():
    """The launch arithmetic of attn_fused.hip restated on the case table: each named branch is taken by the case that claims it."""
    C = RO.CASES
    assert [C[n].B * C[n].H % 8 for n in ("t1", "t9", "h1")] == [4, 1, 1] and {C[n].H for n in ("t9", "h1", "h8", "dpext-groups")} == {3, 1, 8, 32}
    assert all(C[n].T < 64 for n in ("t1", "t9", "t63")) and not C["nomask"].use_mask
    # relattn_dpext_kernel: samples per group, the short last group, tiles skipped by tile_at, negative tile origins (jmin < 0)
    c = C["dpext-groups"]
    n = RO.dpext_bchunk(c.B, c.H, c.T)
    assert n == 2 and c.B % n == 1 and c.B > 1024 // (-(-(2 * c.T - 1) // 128) * c.H)

    def tiles(c):  # (taken, jmin) of every (table block, sample, query block)
        for c0 in range(0, 2 * c.T - 1, 128):
            for ln in c.lens:
                for i0 in range(0, c.T, 64):
                    shift, lim, jmin = c.T - ln, 2 * ln - 1, c0 - (c.T - ln) - c.T + 1 + i0
                    yield not (c0 + 128 <= shift or c0 >= shift + lim or i0 >= ln or jmin + 190 < 0 or jmin >= c.T), jmin
    for name in ("dpext-groups", "t9"):  # (T = 1 has jmin = 0: t1 reaches the clamped rows, not a negative origin)
        took = list(tiles(C[name]))
        assert any(t and j < 0 for t, j in took), name
    assert any(not t for t, _ in tiles(c))
    # forward, STREAM: a query block of real rows whose first processed key block (attn_fused.hip:239-246) is wholly outside some row's window
    c = C["win-5-3"]
    lo, hi = RO.window(c.T, c.chunk, c.hist)
    hit = [(ln, i) for ln in c.lens for i0 in range(0, ln, 64) for i in range(i0, min(i0 + 64, ln))
           if int(lo[i]) >= ((int(lo[i0]) // 64 if i0 + 64 <= ln else 0) + 1) * 64]  # (a partly padded block walks every key block)
    assert hit and int(hi[0]) < 64, "first processed key block fully masked for some rows; window inside one key block"
    assert (int(hi[63]) + 63) // 64 < -(-c.T // 64) and max(c.lens) >= 64, "skipped key blocks (the first query block stops short of the last)"
    # wholly padded query blocks, a partly padded one, shift up to T - 1
    c = C["pad-block"]
    live = RO.live_rows(c.T, c.lens, True)
    assert bool((~live).any()) and any(0 < n % 64 for n in c.lens) and min(c.lens) == 1
    assert RO.CASES["win-wide"].chunk >= RO.CASES["win-wide"].T
