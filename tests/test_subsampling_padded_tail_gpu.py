"""GPU: the subsampling's padded tail computed once (ConformerTransducer._sub_tail_once; DESIGN.md section 2 "Padded tail").

conv2's forward runs over the 256-row blocks that hold real rows (tfasr_gemm_args.row_tiles) and tfasr_s2d_tail_fill copies one
representative row per utterance into the others.  Checked here:
  * the row-tile table in both K-segmented kernels (128-row tiles at N = 64, 256-row tiles at N = 256 and >= 512 blocks): listed blocks
    bitwise what the full product writes, every other row untouched;
  * tfasr_s2d_tail_fill against an index computation on the host;
  * the premise, on the switch-off path: behind the rows the host geometry names, the feature map, a1, o and a2 hold their
    representative row, bit for bit;
  * switch on against switch off: the feature map, a1, o, BatchNorm0's coefficients and moving statistics bitwise equal; BatchNorm1's
    statistics (unordered f32 atomics: two runs of one path differ), a2 and x0 within the bound of that reordering;
  * the f32 model, `sub_norm="layer"` and a shape the fill kernel refuses take the old route.
Batch: B = 5, 400 frames, C = 64 (42 blocks of 256 rows, 14 of them skipped): no tail / real rows ending on a block boundary / mid-block /
shorter than one block / a tail shorter than the convolutions' margins; a time mask ending on the last real frame, two frequency masks."""
import ctypes

import numpy as np
import pytest
import torch

from tensorflowasr_amd import _lib, configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
STEP = 160
T0 = 400
TF = [401, 150, 199, 30, 396]                      # first constant feature frame per utterance
NSAMP = [T0 * STEP] + [t * STEP - 1 for t in TF[1:]]  # ceil((n + 1) / 160) = TF


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32).cpu()


def same(a, b):
    return torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------ the row-tile table, kernel level
def seg_product(dev, M, N, tiles, sentinel):
    """D = A[M, 128] x B[128, N] as two 64-wide K-segments; with `tiles` only those 256-row blocks, over a D prefilled with `sentinel`"""
    g = torch.Generator(device="cpu").manual_seed(M + N)
    A = torch.randn(M, 128, generator=g).to(BF16).to(dev)
    Bm = torch.randn(128, N, generator=g).to(BF16).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    off = torch.tensor([0, 64], dtype=torch.int64, device=dev)
    D = torch.full((M, N), sentinel, dtype=BF16, device=dev)
    rt = None if tiles is None else torch.tensor(tiles, dtype=torch.int32, device=dev)
    K.gemm(A, Bm, D, M, N, 128, 128, N, N, bias=bias, seg=(off, None, 64), row_tiles=rt)
    return D


@pytest.mark.parametrize("M,N", [(800, 64), (1000, 64), (1024, 64), (513 * 256 - 100, 256)])
def test_row_tile_table_computes_listed_blocks_only(dev, M, N):
    nblk = -(-M // 256)
    tiles = sorted({0, nblk - 1} | set(range(2, nblk, 3)))
    full = seg_product(dev, M, N, None, 0.0)
    part = seg_product(dev, M, N, tiles, -7.0)
    blk = torch.arange(M, device=dev) // 256
    listed = torch.isin(blk, torch.tensor(tiles, device=dev))
    assert same(part[listed], full[listed])
    assert bool((part[~listed] == -7.0).all()) and int((~listed).sum()) > 0
    assert bool(torch.isfinite(full.float()).all())


def test_row_tile_table_is_validated(dev):
    A = torch.zeros(1024, 128, dtype=BF16, device=dev)
    Bm = torch.zeros(128, 64, dtype=BF16, device=dev)
    D = torch.zeros(1024, 64, dtype=BF16, device=dev)
    off = torch.tensor([0, 64], dtype=torch.int64, device=dev)
    five = torch.zeros(5, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.TfasrError):  # more entries than blocks
        K.gemm(A, Bm, D, 1024, 64, 128, 128, 64, 64, seg=(off, None, 64), row_tiles=five)
    a = K._gemm_args(A, Bm, D, 1024, 64, 128, 128, 64, 64)  # no K-segments: unsupported, nothing launched
    a.row_tiles, a.n_row_tiles = five.data_ptr(), 2
    assert _lib.load().tfasr_gemm(ctypes.byref(a), None) == _lib.STATUS_UNSUPPORTED


def test_tail_fill_copies_the_representative_row(dev):
    B, T2, F2, C = 3, 30, 6, 16
    rows = B * (T2 + 1) * (F2 + 1)
    x = torch.arange(rows * C, dtype=torch.float32).remainder(251.0).to(BF16).view(rows, C).to(dev)
    nblk = -(-rows // 256)
    tiles, rep = [1, nblk - 1], [4, 9, 17]
    want = x.clone()
    r = torch.arange(rows, device=dev)
    b, ff = r // ((T2 + 1) * (F2 + 1)), r % (F2 + 1)
    src = (b * (T2 + 1) + torch.tensor(rep, device=dev)[b]) * (F2 + 1) + ff
    hit = torch.isin(r // 256, torch.tensor(tiles, device=dev))
    want[hit] = x[src[hit]]
    K.s2d_tail_fill(x, torch.tensor(tiles, dtype=torch.int32, device=dev), torch.tensor(rep, dtype=torch.int32, device=dev), B, T2, F2, C)
    assert same(x, want)
    with pytest.raises(_lib.TfasrUnsupported):
        K.s2d_tail_fill(x.float(), torch.tensor(tiles, dtype=torch.int32, device=dev), torch.tensor(rep, dtype=torch.int32, device=dev), B, T2, F2, C)


# ------------------------------------------------------------------------------------------------ the model
def batch(dev):
    g = np.random.default_rng(7)
    sig = np.zeros((5, T0 * STEP), np.float32)
    for b, n in enumerate(NSAMP):
        sig[b, :n] = np.clip(g.standard_normal(n) * 0.1, -1, 1)
    fm = np.zeros((5, 1, 2), np.int32)
    fm[2, 0], fm[3, 0] = (10, 7), (60, 20)
    tm = np.zeros((5, 1, 2), np.int32)
    tm[1, 0] = (140, 10)  # ends on utterance 1's last real frame (149)
    tm[0, 0] = (200, 15)
    return torch.from_numpy(sig).to(dev), (torch.from_numpy(fm), torch.from_numpy(tm))


def run(dev, on, dtype=BF16, **over):
    cfg = configs.conformer_tiny(filters=64, num_blocks=1, **over)
    model = ConformerTransducer(cfg, dev, dtype=dtype, seed=0)
    model._sub_tail_once = on
    sig, masks = batch(dev)
    feats, flen = model.frontend(sig, NSAMP, True, masks)
    ctx = {}
    x0, T2, elen = model._subsampling_fwd(feats, flen, True, ctx)
    torch.cuda.synchronize()
    s = ctx["sub"]
    out = dict(feats=feats, x0=x0)
    if s.get("s2d"):
        out.update(a1=s["a1"], o=s["o"], a2=s["a2"], fin0=s["bn0"][0], fin1=s["bn1"][0])
    for nm in ("enc/sub/bn0", "enc/sub/bn1"):
        if nm + "/mm" in model.ps.state:
            out[nm + "/mm"], out[nm + "/mv"] = model.ps.state[nm + "/mm"], model.ps.state[nm + "/mv"]
    took = [k for k, v in model._consts.items() if isinstance(k, tuple) and k[:1] == ("tail",) and v is not None]
    return {k: v.clone() for k, v in out.items()}, bool(took), model


@pytest.fixture(scope="module")
def off(dev):
    return run(dev, False)[0]


def test_premise_padded_rows_hold_their_representative_row(dev, off):
    rows = ConformerTransducer._tail_rows(np.array(TF), T0)
    T2, F2, C = 100, 20, 64
    f = off["feats"]
    assert f.shape == (5, T0, 80)
    seen = 0
    for b in range(5):
        t = int(rows["feats"][b])
        if t < T0:
            assert same(f[b, t:], f[b, t:t + 1].expand(T0 - t, -1)), b
            seen += 1
        for name, width in (("a1", 4 * C), ("o", C), ("a2", C)):
            x = off[name].view(5, T2 + 1, F2 + 1, width)
            tt = int(rows[name][b])
            if tt <= T2:
                assert same(x[b, tt:], x[b, tt:tt + 1].expand(T2 + 1 - tt, -1, -1)), (name, b)
                seen += 1
    assert seen == 4 + 3 * 3  # utterance 0 has no tail at all, utterance 4 one in the feature map only
    # ... and the geometry is not vacuous: the row in front of a tail differs from it
    o = off["o"].view(5, T2 + 1, F2 + 1, C)
    assert not same(o[1, int(rows["o"][1]) - 3, 1:], o[1, int(rows["o"][1]), 1:])


# what no unordered sum feeds: bitwise.  BatchNorm1's batch sums are f32 atomics of up to P = 1024 per-workgroup partial sums in arrival
# order (csrc/norm.hip), so two runs of ONE path already differ there (measured in the same process: coefficients by 1.4e-6, a2 and x0 by
# one bf16 step); what they feed is held to the reordering bound P * 2^-24 = 6e-5 of a unit-scale mean, rounded up to 1e-4, and to what
# that bound lets through the elementwise maps behind it.
EXACT = ("feats", "a1", "o", "fin0", "enc/sub/bn0/mm", "enc/sub/bn0/mv")
STATS = ("fin1", "enc/sub/bn1/mm", "enc/sub/bn1/mv")


def forward_agrees(got, ref, model):
    assert sorted(got) == sorted(ref) == sorted(EXACT + STATS + ("a2", "x0"))
    for k in EXACT:
        assert same(got[k], ref[k]), k
    for k in STATS:
        d = (got[k] - ref[k]).abs()
        print(k, "max difference", float(d.max()))
        assert bool((d <= 1e-4 * (1 + ref[k].abs())).all()), k
    # a2 = swish(o * scale + shift) in bf16: |swish'| <= 1.1, then one rounding step (2^-8 relative, 2^-7 across a binade edge)
    a2g, a2r, o = got["a2"].float(), ref["a2"].float(), ref["o"].float()
    d2 = (a2g - a2r).abs()
    print("a2 max difference", float(d2.max()), "elements that differ", int((d2 > 0).sum()), "of", d2.numel())
    assert bool((d2 <= 1.1e-4 * (1 + o.abs()) + 2.0 ** -7 * a2r.abs()).all())
    # x0 = a2 (as [B T2, F2 C] rows) @ W + bias, f32 accumulation in one fixed order, one bf16 rounding
    W = model.ps.w2d("enc/linear/w").float().abs()
    rows = d2.view(5, 101, 21, 64)[:, 1:, 1:].reshape(500, 20 * 64)
    dx = (got["x0"].float() - ref["x0"].float()).abs()
    print("x0 max difference", float(dx.max()))
    assert bool((dx <= rows @ W + 2.0 ** -7 * ref["x0"].float().abs()).all())
    assert bool(torch.isfinite(got["x0"].float()).all())


def test_forward_is_bitwise_the_full_computation(dev, off):
    on, took, model = run(dev, True)
    assert took  # the tables were built and used: 14 of 42 blocks skipped
    comp, skip, rep = ConformerTransducer._tail_blocks(np.array(TF), 5, T0, 100, 20)
    assert len(skip) == 14 and 21 in skip and 20 in comp  # utterance 2's real rows end on the boundary of blocks 20 | 21
    forward_agrees(on, off, model)


def test_f32_layer_norm_and_refused_shapes_take_the_full_route(dev, off, monkeypatch):
    r32, took32, _ = run(dev, True, dtype=torch.float32)
    assert not took32 and bool(torch.isfinite(r32["x0"]).all())
    rl, tookl, _ = run(dev, True, sub_norm="layer")
    assert not tookl and "o" not in rl and bool(torch.isfinite(rl["x0"].float()).all())

    calls = []

    def fill(*a, **k):
        calls.append(1)
        raise _lib.TfasrUnsupported("refused")

    monkeypatch.setattr(K, "s2d_tail_fill", fill)
    ru, _, model = run(dev, True)
    assert calls == [1]
    forward_agrees(ru, off, model)
