"""CPU: the host geometry of the subsampling's padded tail (ConformerTransducer._tail_rows / _tail_blocks) against a brute-force
propagation of "this row only reads constant rows" through the two causal 3x3 stride-2 convolutions and the haloed space-to-depth layout
(csrc/conv2d.hip: output row t reads input rows 2t-2 .. 2t; S row tt holds t1 = 2tt-2 and 2tt-1)."""
import numpy as np
import pytest

from tensorflowasr_amd.conformer import ConformerTransducer as M


def brute(tf, T0):
    """first constant row of conv1's output, of the S layout's time rows and of conv2's output, by propagation (T2 + 1 = none)"""
    T1 = (T0 + 1) // 2
    T2 = (T1 + 1) // 2
    cf = np.arange(T0) >= tf
    c1 = np.array([2 * t - 2 >= 0 and all(cf[ti] for ti in range(2 * t - 2, 2 * t + 1) if ti < T0) for t in range(T1)])
    # S row tt (1 .. T2): both time parities; the slot past an odd T1 is zero, not the representative value
    cs = np.zeros(T2 + 1, bool)
    for tt in range(1, T2 + 1):
        a, b = 2 * tt - 2, 2 * tt - 1
        cs[tt] = c1[a] and b < T1 and c1[b]
    co = np.zeros(T2 + 1, bool)
    for tt in range(2, T2 + 1):
        co[tt] = c1[2 * tt - 4] and c1[2 * tt - 3] and c1[2 * tt - 2]
    return c1, cs, co


@pytest.mark.parametrize("T0", [400, 401, 402, 403, 37])
def test_tail_rows_only_name_rows_that_read_constant_rows(T0):
    T1 = (T0 + 1) // 2
    T2 = (T1 + 1) // 2
    tfs = np.arange(1, T0 + 3)
    rows = M._tail_rows(tfs, T0)
    assert (rows["feats"] == tfs).all() and (rows["a2"] == rows["o"]).all()
    for tf, a1, o in zip(tfs, rows["a1"], rows["o"]):
        c1, cs, co = brute(tf, T0)
        # sound: every row the tables call constant reads constant rows only (the S layout's last row may hold the zero slot of an
        # odd T1 in its second time parity - conv2 never reads that slot, but the row is not claimed for a1 either way)
        for tt in range(int(a1), T2 + 1):
            assert cs[tt] or (tt == T2 and T1 % 2 == 1 and c1[2 * tt - 2]), (tf, tt)
        for tt in range(int(o), T2 + 1):
            assert co[tt], (tf, tt)
        # and not wasteful: at most two rows later than the first row that could be called constant
        first = next((tt for tt in range(2, T2 + 1) if co[tt:].all()), T2 + 1)
        assert o - first <= 2, (tf, o, first)


@pytest.mark.parametrize("B,T0,F2", [(5, 400, 20), (3, 403, 20), (4, 90, 7), (1, 400, 20)])
def test_tail_blocks_partition_the_rows(B, T0, F2):
    T1 = (T0 + 1) // 2
    T2 = (T1 + 1) // 2
    g = np.random.default_rng(B * 1000 + T0)
    for _ in range(20):
        tf = g.integers(1, T0 + 3, B)
        comp, skip, rep = M._tail_blocks(tf, B, T0, T2, F2)
        rows = B * (T2 + 1) * (F2 + 1)
        nblk = -(-rows // 256)
        assert sorted(np.concatenate([comp, skip]).tolist()) == list(range(nblk))
        o = M._tail_rows(tf, T0)["o"]
        r = np.arange(nblk * 256)
        b, tt = r // ((T2 + 1) * (F2 + 1)), r // (F2 + 1) % (T2 + 1)
        inside = r < rows
        bb = np.minimum(b, B - 1)
        assert ((rep >= 1) & (rep <= T2)).all()
        # a skipped block holds halo rows and rows BEHIND the representative row only; that row is a constant one
        skipped = np.isin(r // 256, skip) & inside
        assert ((tt[skipped] == 0) | ((tt[skipped] > rep[bb[skipped]]) & (rep[bb[skipped]] >= o[bb[skipped]]))).all()
        # every real row, the representative rows included, lies in a computed block
        real = inside & (tt >= 1) & (tt <= np.where(o + 1 <= T2, o, T2)[bb])
        assert np.isin(r[real] // 256, comp).all()
        # nothing is computed for nothing: a computed block holds at least one real row
        assert set(comp.tolist()) == set((r[real] // 256).tolist())
