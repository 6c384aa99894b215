"""tfasr_decode_update_detail (csrc/decode.hip: the register kernels NV = 4 / 8 / 16 and the generic kernel with their DETAIL flag) alone,
through K.decode_update_detail, against the float64 recorder of tests/recognize_detail_oracle.py evaluated on the same logits (for bf16:
on the bf16-rounded values).

What is held: the integer state and h, c are bit-equal to K.decode_update on the same inputs; tok_frames is exactly the oracle's; the
detail buffers change at exactly the columns where a symbol is written; tok_logp and tok_entropy meet the project's single-layer f32 bar
(rtol 1e-4 / atol 1e-5, BAR of tests/test_decode_step_gpu.py).  Every test first asserts on the CPU that plain torch float32 stays under
half that bar on its inputs and that no row's decision hangs on a last-digit difference (a clear top-2 margin, or an exact tie).  The
worst ratios go to profiles/recognize_detail_parity.json."""
import math

import numpy as np
import pytest
import torch

from tensorflowasr_amd import kernels as K

import decode_oracle as DO
import recognize_detail_oracle as RD

pytestmark = pytest.mark.gpu
ST_KEYS = ("nframes", "frame_idx", "prev_tok", "tok_idx", "tokens", "per_frame", "h", "c")
SENTINEL = dict(frames=-1, logp=7.5, entropy=-7.5)  # what the caller put there: values the kernel never produces
TIES = [(300, 513), (70, 259), (255, 256), (1023, 1024)]
F32, BF16 = torch.float32, torch.bfloat16
# V, P, logits type: the register kernels' three widths and their edges; the generic kernel by V, by P and by type
CASES = [(8, 640, F32), (1000, 640, F32), (1024, 640, F32), (1025, 640, F32), (2048, 640, F32), (2049, 640, F32), (4096, 640, F32),
         (4097, 24, F32), (1500, 1028, F32), (1000, 640, BF16)]
ROWS = [1, 17, 65]
_PARITY = {}


def _cid(V, P, dtype, B=None):
    return f"V={V} P={P} {'bf16' if dtype == BF16 else 'f32'}" + (f" B={B}" if B is not None else "")


@pytest.fixture(scope="module", autouse=True)
def parity_profile():
    yield
    if {_cid(*c, B) for c in CASES for B in ROWS} <= set(_PARITY):  # (a partial run leaves the file alone)
        RD.write_parity("decode_update_detail", _PARITY)


def _state_to_dev(dev, st, dtype):
    return {k: torch.from_numpy(np.ascontiguousarray(st[k])).to(F32 if k == "c" else dtype if k == "h" else torch.int32).to(dev) for k in ST_KEYS}


def _det_to_dev(dev, det):
    return [torch.from_numpy(np.ascontiguousarray(det["frames"])).to(torch.int32).to(dev), torch.from_numpy(np.ascontiguousarray(det["logp"])).to(F32).to(dev),
            torch.from_numpy(np.ascontiguousarray(det["entropy"])).to(F32).to(dev)]


def run(dev, mode, logits, st, det, h_new, c_new, max_tokens, act=1, mtpf=3):
    """K.decode_update_detail and K.decode_update on device copies of the same state -> (state, detail buffers), read back; asserts the two states bit-equal.
    `logits` is a torch tensor of the type under test; h / h_new take that type, c / c_new are f32."""
    dtype = logits.dtype
    lg = logits.to(dev).contiguous()
    hn, cn = torch.as_tensor(h_new).to(dtype).to(dev).contiguous(), torch.as_tensor(c_new).to(F32).to(dev).contiguous()
    out = []
    for detail in (True, False):
        d = _state_to_dev(dev, st, dtype)
        active = torch.tensor([act], dtype=torch.int32, device=dev)
        args = (lg, active, d["nframes"], d["frame_idx"], d["prev_tok"], d["tok_idx"], d["tokens"], d["per_frame"], hn, cn, d["h"], d["c"])
        if detail:
            bufs = _det_to_dev(dev, det)
            K.decode_update_detail(*args, *bufs, max_tokens, 0, mode, mtpf)
        else:
            K.decode_update(*args, max_tokens, 0, mode, mtpf)
        torch.cuda.synchronize()
        assert int(active.item()) == act
        out.append({k: d[k].cpu() for k in ST_KEYS})
    got, plain = out
    for k in ST_KEYS:  # bit-equal to the plain entry point (h, c compared as raw bits through torch.equal on equal dtypes)
        assert got[k].dtype == plain[k].dtype and torch.equal(got[k].view(torch.int16 if got[k].dtype == BF16 else torch.int32),
                                                              plain[k].view(torch.int16 if plain[k].dtype == BF16 else torch.int32)), k
    return got, dict(frames=bufs[0].cpu().numpy(), logp=bufs[1].cpu().numpy(), entropy=bufs[2].cpu().numpy())


def sentinel_detail(shape):
    return dict(frames=np.full(shape, SENTINEL["frames"], np.int64), logp=np.full(shape, SENTINEL["logp"], np.float64),
                entropy=np.full(shape, SENTINEL["entropy"], np.float64))


def f32_on_cpu_is_within_half_the_bar(logits):
    """the condition on the inputs: float32 log-softmax and entropy of every row against float64 stay under half the bar"""
    x = logits.float()
    l64, l32 = torch.log_softmax(x.double(), -1), torch.log_softmax(x, -1)
    top = l64.argmax(-1, keepdim=True)
    r_lp = RD.ratio(l32.gather(1, top).numpy(), l64.gather(1, top).numpy())
    r_h = RD.ratio(RD.entropy(l32).numpy(), RD.entropy(l64).numpy())
    assert r_lp <= 0.5 and r_h <= 0.5, (r_lp, r_h)
    return r_lp, r_h


def check(dev, mode, logits, st, det, h_new, c_new, max_tokens, T, mtpf=3, act=1):
    """one call against the oracle -> (detail buffers read back, written [B], worst ratios (logp, entropy))"""
    exp_st, exp_det, written = (RD.update_detail(mode, logits, st, det, h_new, c_new, max_tokens, T, max_tokens_per_frame=mtpf) if act
                                else (st, det, np.zeros(logits.shape[0], bool)))
    got_st, got_det = run(dev, mode, logits, st, det, h_new, c_new, max_tokens, act, mtpf)
    for k in ST_KEYS[:6]:
        np.testing.assert_array_equal(got_st[k].numpy(), exp_st[k], err_msg=k)
    np.testing.assert_array_equal(got_det["frames"], exp_det["frames"])
    changed = exp_det["frames"] != det["frames"]
    changed |= (exp_det["logp"] != det["logp"])  # (an overwritten column may keep its frame)
    for k in ("logp", "entropy"):  # the columns no symbol went to hold what the caller put there, bit for bit
        np.testing.assert_array_equal(got_det[k][~changed], np.asarray(det[k], np.float32)[~changed], err_msg=k)
        assert np.isfinite(got_det[k]).all(), k
    r = (RD.ratio(got_det["logp"][changed], exp_det["logp"][changed]), RD.ratio(got_det["entropy"][changed], exp_det["entropy"][changed]))
    assert r[0] <= 1.0 and r[1] <= 1.0, r
    return got_det, written, r


def make_rows(g, B, V, dtype):
    """B rows of eight kinds (b % 8) -> (logits of `dtype`, expected symbol per row or None, kind per row)"""
    rows, want, kinds = [], [], []
    ties = [t for t in TIES if t[1] < V]
    for b in range(B):
        kind = b % 8
        if kind == 3 and not ties:
            kind = 0
        if kind in (0, 1, 6):  # a wide, a nearly flat and a unit-scale row, the maximum raised clear of the runner-up (bf16 rounding included)
            scale = {0: 3.0, 1: 0.01, 6: 1.0}[kind]
            r = torch.randn(V, generator=g) * scale
            r[0] = r.min() - scale  # (not the blank)
            r[r.argmax()] += 0.17 * scale
            w = None
        elif kind == 2:  # a blank: nothing is written
            r = torch.randn(V, generator=g)
            r[0] = 20.0
            w = 0
        elif kind == 3:  # an exact tie: the lower index, with the tied value
            lo, hi = ties[(b // 8) % len(ties)]
            r = torch.randn(V, generator=g)
            r[lo] = r[hi] = 9.5
            w = lo
        elif kind == 4:  # every class but one at -1e4: probability 1, entropy 0
            r = torch.full((V,), -1e4)
            r[min(5, V - 1)] = 3.0
            w = min(5, V - 1)
        elif kind == 5:  # classes of probability exactly 0, the blank among them
            r = torch.randn(V, generator=g) * 2
            r[torch.arange(0, V, 3)] = -math.inf
            r[1] += 0.5  # (index 1 survives: V >= 8)
            r[r.argmax()] += 0.4
            w = None
        else:  # the last class, alone on its stride
            r = torch.randn(V, generator=g)
            r[V - 1] = 12.0
            w = V - 1
        rows.append(r)
        want.append(w)
        kinds.append(kind)
    logits = torch.stack(rows).to(dtype)
    x = logits.float()
    top = x.topk(3 if V >= 3 else 2, -1).values
    for b, kind in enumerate(kinds):  # no decision hangs on a last digit: a clear margin, or an exact tie above a clear third
        if kind == 3:
            assert top[b, 0] == top[b, 1] and top[b, 1] - top[b, 2] > 1e-2
        else:
            assert top[b, 0] - top[b, 1] > 1e-3, (b, kind)
        if want[b] is None:
            want[b] = int(x[b].argmax())
            assert want[b] != 0
    return logits, want, kinds


@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("V,P,dtype", CASES, ids=[_cid(*c) for c in CASES])
def test_values_ties_and_extreme_rows(dev, V, P, dtype, B):
    g = torch.Generator().manual_seed(V * 7 + P + B)
    logits, want, kinds = make_rows(g, B, V, dtype)
    cpu = f32_on_cpu_is_within_half_the_bar(logits)
    T, max_tokens = 5, 11
    rnd = lambda: torch.randn(B, P, generator=g).to(dtype).float().numpy()
    h, c, h_new, c_new = rnd(), torch.randn(B, P, generator=g).numpy(), rnd(), torch.randn(B, P, generator=g).numpy()
    fi = np.arange(B) % 5
    fi[np.asarray(kinds) == 6] = 5  # a finished row that still emits: it records its last frame
    st = dict(nframes=np.full(B, 5), frame_idx=fi, prev_tok=np.full(B, 3), tok_idx=1 + np.arange(B) % 4, tokens=np.full((B, max_tokens), 7),
              per_frame=np.zeros(B, np.int64), h=h, c=c)
    det = sentinel_detail((B, max_tokens))
    got, written, r = check(dev, 0, logits, st, det, h_new, c_new, max_tokens, T)
    l64 = torch.log_softmax(logits.double(), -1)
    for b in range(B):
        col = st["tok_idx"][b] + 1
        assert written[b] == (want[b] != 0)
        if not written[b]:
            continue
        assert got["frames"][b, col] == (4 if kinds[b] == 6 else fi[b])
        assert RD.ratio(got["logp"][b, col], float(l64[b, want[b]])) <= 1.0  # the lower index of a tie, with the tied value
        if kinds[b] == 4:
            assert got["logp"][b, col] == 0.0 and got["entropy"][b, col] == 0.0
        if kinds[b] == 5:
            assert math.isfinite(got["entropy"][b, col]) and got["entropy"][b, col] > 0
    assert (got["frames"] >= 0).sum() == written.sum()
    check(dev, 0, logits, st, det, h_new, c_new, max_tokens, T, act=0)  # active = 0: nothing is written anywhere
    _PARITY[_cid(V, P, dtype, B)] = dict(tok_logp=r[0], tok_entropy=r[1], cpu_f32_logp=cpu[0], cpu_f32_entropy=cpu[1])


def _spiked(g, B, V, cur, dtype):
    logits = torch.randn(B, V, generator=g)
    logits[torch.arange(B), torch.as_tensor(cur)] = 15.0
    return logits.to(dtype)


def _rand_state(g, B, P, dtype):
    return [torch.randn(B, P, generator=g).to(dtype if i % 2 == 0 else F32).float().numpy() for i in range(4)]  # h, c, h_new, c_new


VARIANTS = [(40, 24, F32), (4097, 24, F32), (1500, 1028, F32), (1000, 640, BF16)]  # register kernel; generic by V, by P, by type
VIDS = [_cid(*v) for v in VARIANTS]


@pytest.mark.parametrize("V,P,dtype", VARIANTS, ids=VIDS)
def test_detail_bookkeeping_mode_0(dev, V, P, dtype):
    """the table of test_update_bookkeeping_mode_0: details at exactly the columns a symbol goes to, the last column overwritten with its
    details, a finished row (fi == nf) recording frame nf - 1; fi == nf + 1 is a forced blank and, like every blank, writes nothing"""
    g = torch.Generator().manual_seed(V + P)
    max_tokens, T = 7, 5
    #        blank  symbol  ->col 6  stays 6  ti>=max  fi>nf   fi==nf  blank at ti = max
    cur = [0, 5, 6, 8, 9, 10, 11, 0]
    ti = [3, 3, 5, 6, 7, 2, 2, 7]
    fi = [2, 2, 0, 1, 1, 5, 4, 4]
    nf = [5, 5, 5, 5, 5, 4, 4, 4]
    B = len(cur)
    h, c, h_new, c_new = _rand_state(g, B, P, dtype)
    st = dict(nframes=np.array(nf), frame_idx=np.array(fi), prev_tok=np.full(B, 3), tok_idx=np.array(ti), tokens=np.full((B, max_tokens), 33),
              per_frame=np.zeros(B, np.int64), h=h, c=c)
    det = sentinel_detail((B, max_tokens))
    det["frames"][3, 6], det["logp"][3, 6], det["entropy"][3, 6] = 0, -9.0, 9.0  # the token that sat in the last column before
    logits = _spiked(g, B, V, cur, dtype)
    f32_on_cpu_is_within_half_the_bar(logits)
    got, written, _ = check(dev, 0, logits, st, det, h_new, c_new, max_tokens, T)
    assert written.tolist() == [False, True, True, True, False, False, True, False]
    cells = {(1, 4): 2, (2, 6): 0, (3, 6): 1, (6, 3): 3}
    assert {(int(b), int(k)) for b, k in zip(*np.nonzero(got["frames"] != -1))} == set(cells)
    for (b, k), frame in cells.items():
        assert got["frames"][b, k] == frame and -1e-2 < got["logp"][b, k] < 0 and 0 < got["entropy"][b, k] < 0.1
    check(dev, 0, logits, st, det, h_new, c_new, max_tokens, T, act=0)


@pytest.mark.parametrize("V,P,dtype", VARIANTS, ids=VIDS)
def test_detail_bookkeeping_mode_1(dev, V, P, dtype):
    """the utterance of test_update_bookkeeping_mode_1, iteration by iteration: three symbols on one frame share it, and the blank that
    re-writes tokens[tok_idx] leaves that column's details alone"""
    g = torch.Generator().manual_seed(V + P + 1)
    nframes, mtpf = 4, 3
    max_tokens = nframes * mtpf
    st = DO.new_state(1, 1, P, [nframes], max_tokens)
    st["h"], st["c"] = _rand_state(g, 1, P, dtype)[:2]
    st["prev_tok"][:] = 4
    det = sentinel_detail((1, max_tokens))
    seq = [0, 5, 6, 7, 0, 8, 0, 9, 0]
    for it, cur in enumerate(seq):
        act = int(DO.active(1, st["nframes"], st["frame_idx"], st["tok_idx"], max_tokens))
        assert act == (1 if it < 7 else 0)
        if it == 4:
            st["tokens"][0, st["tok_idx"][0]] = 33  # this iteration's blank writes prev_tok back over it ...
            det["logp"][0, st["tok_idx"][0]] = -3.25  # ... and must not touch the details beside it
        _, _, h_new, c_new = _rand_state(g, 1, P, dtype)
        logits = _spiked(g, 1, V, [cur], dtype)
        exp_st, exp_det, written = RD.update_detail(1, logits, st, det, h_new, c_new, max_tokens, nframes, max_tokens_per_frame=mtpf) if act else (st, det, [False])
        got, _, _ = check(dev, 1, logits, st, det, h_new, c_new, max_tokens, nframes, mtpf=mtpf, act=act)
        assert bool(written[0]) == (act == 1 and cur != 0)
        st, det = exp_st, {k: np.asarray(got[k], np.float64 if k != "frames" else np.int64) for k in got}  # carry the device's buffers on
        np.testing.assert_array_equal(det["frames"], exp_det["frames"])
    assert st["tokens"][0].tolist() == [5, 6, 7, 8] + [0] * 8
    assert det["frames"][0].tolist() == [1, 1, 1, 3] + [-1] * 8 and det["logp"][0, 2] == -3.25
    assert (det["logp"][0, 4:] == SENTINEL["logp"]).all() and (det["entropy"][0, 4:] == SENTINEL["entropy"]).all()


@pytest.mark.parametrize("V,P,dtype", VARIANTS, ids=VIDS)
def test_detail_bookkeeping_mode_2(dev, V, P, dtype):
    """the table of test_update_bookkeeping_mode_2: finished rows, a blank and the symbol dropped past the buffer write no details"""
    g = torch.Generator().manual_seed(V + P + 2)
    max_tokens, mtpf, T = 6, 3, 6
    #      finished  blank: reset  symbol  third symbol  dropped  past the end
    cur = [9, 0, 5, 6, 7, 8]
    fi = [4, 1, 1, 1, 1, 6]
    nf = [4, 4, 4, 4, 4, 4]
    pf = [1, 2, 0, 2, 0, 2]
    ti = [2, 2, 2, 2, 5, 2]
    B = len(cur)
    h, c, h_new, c_new = _rand_state(g, B, P, dtype)
    st = dict(nframes=np.array(nf), frame_idx=np.array(fi), prev_tok=np.full(B, 3), tok_idx=np.array(ti), tokens=np.full((B, max_tokens), 33),
              per_frame=np.array(pf), h=h, c=c)
    det = sentinel_detail((B, max_tokens))
    logits = _spiked(g, B, V, cur, dtype)
    f32_on_cpu_is_within_half_the_bar(logits)
    got, written, _ = check(dev, 2, logits, st, det, h_new, c_new, max_tokens, T, mtpf=mtpf)
    assert written.tolist() == [False, False, True, True, False, False]
    assert {(int(b), int(k)) for b, k in zip(*np.nonzero(got["frames"] != -1))} == {(2, 3), (3, 3)}
    assert got["frames"][2, 3] == 1 and got["frames"][3, 3] == 1
    check(dev, 2, logits, st, det, h_new, c_new, max_tokens, T, mtpf=mtpf, act=0)
