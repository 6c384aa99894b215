"""tfasr_attn_plain_fwd (csrc/attn_plain.hip) and tfasr_add_pe against the float64 oracle of tests/transformer_oracle.py, on operands rounded
to the kernel's storage type.  B = 3, H = 2.

  T        1, 63, 64, 65, 130, 257: a single row, one short of a block, an exact block, one past it, a ragged tail, several blocks
  lengths  two sets per case, [0, 1, T] and [mid, T, 0] with mid = max(1, 2 T // 3), which ends inside a block at every T
  masks    none; causal; (chunk, hist) = (16, 64) the shipped window, (3, 5) not aligned to the tile, (4, 0) no history, (16, -1) unlimited.
           At T = 257 whole key blocks fall outside every window of a query block; with the mid-block length and (16, 64) padded rows
           (which read every key) sit beside skipped key blocks.
  types    bf16 at dh 64 and 128 (the MFMA kernel), f32 at dh 16, 64 and 128 (the FMA twin)

Bars.  f32: the largest absolute error of the ORACLE'S OWN arithmetic run in float32 by torch on the CPU on the same operands, times 4 for
the summation order.  bf16: the rounding floor - the float64 oracle with the probabilities rounded to bf16 before P V and its result
rounded to bf16, relative (Frobenius) error against the unrounded oracle - times 2, the method of tests/test_ds2_gpu.py.  lse is an f32
result in both types (f32 sums of exact products in the bf16 kernel): 4 times the f32 oracle's error, where that error is taken as at least
one spacing of float32 at the largest |lse| of the case - at T = 1 torch's float32 result can be exact, and no f32 store can be asked for
less than the format holds.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

from tensorflowasr_amd import _lib
from tensorflowasr_amd import kernels as K

import transformer_oracle as TO

pytestmark = pytest.mark.gpu
B, H = 3, 2
TS = [1, 63, 64, 65, 130, 257]
MASKS = {"none": dict(), "causal": dict(causal=True), "w16_64": dict(chunk=16, hist=64), "w3_5": dict(chunk=3, hist=5),
         "w4_0": dict(chunk=4, hist=0), "w16_inf": dict(chunk=16, hist=-1)}
_CACHE = {}


def _lens(T):
    return [[0, 1, T], [max(1, 2 * T // 3), T, 0]]


def _operands(T, dh, dtype):
    g = torch.Generator().manual_seed(T * 1000 + dh)
    qkv = torch.randn(B * T, 3 * H * dh, generator=g)
    qkv[:, :H * dh] *= 2.0  # scores of a few units at scale 1 / sqrt(dh): far from a uniform softmax
    return qkv.to(dtype)


def _reference(T, dh, dtype, mask, li):
    """f64 oracle (out, lse), and per type the yardstick: the f32 run's errors / the bf16 floor - computed once per case"""
    key = (T, dh, dtype, mask, li)
    if key not in _CACHE:
        qkv, lens, kw = _operands(T, dh, dtype), _lens(T)[li], MASKS[mask]
        scale = 1.0 / math.sqrt(dh)
        out, lse = TO.attention_qkv(qkv.double(), B, H, T, dh, scale, lens=lens, want_lse=True, **kw)
        o32, l32 = TO.attention_qkv(qkv.float(), B, H, T, dh, scale, lens=lens, want_lse=True, **kw)
        rec = dict(out=out, lse=lse, err32=float((o32.double() - out).abs().max()), lse_err32=float((l32.double() - lse).abs().max()))
        if dtype == torch.bfloat16:
            fl = TO.bf16_round(TO.attention_qkv(qkv.double(), B, H, T, dh, scale, lens=lens, pround=TO.bf16_round, **kw))
            rec["floor"] = float(torch.sqrt(((fl - out) ** 2).sum() / (out ** 2).sum()))
        _CACHE[key] = rec
    return _CACHE[key]


def _run(dev, T, dh, dtype, mask, li, use_mask=True):
    kw = MASKS[mask]
    qkv = _operands(T, dh, dtype).to(dev)
    lens = torch.tensor(_lens(T)[li], dtype=torch.int32, device=dev)
    out, lse = K.attn_plain_fwd(qkv, lens, B, H, T, dh, 1.0 / math.sqrt(dh), use_mask=use_mask, causal=kw.get("causal", False),
                                chunk_size=kw.get("chunk"), history_size=kw.get("hist"), want_lse=True)
    plain = K.attn_plain_fwd(qkv, lens, B, H, T, dh, 1.0 / math.sqrt(dh), use_mask=use_mask, causal=kw.get("causal", False),
                             chunk_size=kw.get("chunk"), history_size=kw.get("hist"))
    torch.cuda.synchronize()
    assert torch.equal(plain, out)  # lse = NULL changes nothing
    return out.double().cpu(), lse.double().cpu()


def _lse_bar(ref):
    return 4 * max(ref["lse_err32"], float(np.spacing(np.float32(ref["lse"].abs().max()))))


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dh", [16, 64, 128])
def test_f32_twin(dev, dh, T, mask):
    for li in (0, 1):
        ref = _reference(T, dh, torch.float32, mask, li)
        out, lse = _run(dev, T, dh, torch.float32, mask, li)
        err, lerr = float((out - ref["out"]).abs().max()), float((lse - ref["lse"]).abs().max())
        print(f"f32 dh {dh} T {T} {mask} lens {_lens(T)[li]}: error {err:.3e} (f32 oracle {ref['err32']:.3e}), lse {lerr:.3e} (f32 oracle {ref['lse_err32']:.3e})")
        assert torch.isfinite(out).all() and err <= 4 * ref["err32"] and lerr <= _lse_bar(ref)


@pytest.mark.parametrize("mask", list(MASKS))
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("dh", [64, 128])
def test_bf16_kernel(dev, dh, T, mask):
    for li in (0, 1):
        ref = _reference(T, dh, torch.bfloat16, mask, li)
        out, lse = _run(dev, T, dh, torch.bfloat16, mask, li)
        err = float(torch.sqrt(((out - ref["out"]) ** 2).sum() / (ref["out"] ** 2).sum()))
        lerr = float((lse - ref["lse"]).abs().max())
        print(f"bf16 dh {dh} T {T} {mask} lens {_lens(T)[li]}: relative error {err:.3e} (floor {ref['floor']:.3e}), lse {lerr:.3e} (f32 oracle {ref['lse_err32']:.3e})")
        assert torch.isfinite(out).all() and err <= 2 * ref["floor"] and lerr <= _lse_bar(ref)


@pytest.mark.parametrize("dtype,dh", [(torch.float32, 16), (torch.bfloat16, 128)])
def test_padded_rows_are_uniform_over_all_keys_and_valid_rows_see_only_their_window(dev, dtype, dh):
    """the properties themselves, at T = 130 with the mid-block length and the (16, 64) window: a padded row equals the mean of ALL value
    rows whatever the window; a valid row does not change when a key outside its window changes"""
    T, li = 130, 1
    lens = _lens(T)[li]
    out, lse = _run(dev, T, dh, dtype, "w16_64", li)
    qkv = _operands(T, dh, dtype)
    v = qkv[:, 2 * H * dh:].double().reshape(B, T, H * dh)
    tol = 2.0 ** -7 if dtype == torch.bfloat16 else 1e-5
    o = out.reshape(B, T, H * dh)
    for b, n in enumerate(lens):
        if n < T:
            assert float((o[b, n:] - v[b].mean(0)[None]).abs().max()) <= tol * float(v[b].abs().max())
            assert np.allclose(lse.reshape(B, H, T)[b, :, n:].numpy(), math.log(T), rtol=0, atol=1e-5)
    # key 0 lies outside the window of every query from chunk 80 on (80 - 64 = 16 > 0): poison it and those valid rows keep their bits
    q2 = qkv.clone().reshape(B, T, 3 * H * dh)
    q2[:, 0, H * dh:] = 50.0
    q2 = q2.reshape(B * T, 3 * H * dh).to(dev)
    out2 = K.attn_plain_fwd(q2, torch.tensor(lens, dtype=torch.int32, device=dev), B, H, T, dh, 1.0 / math.sqrt(dh), chunk_size=16, history_size=64)
    o2 = out2.double().cpu().reshape(B, T, H * dh)
    assert torch.equal(o2[1, 80:], o[1, 80:]) and not torch.equal(o2[1, :16], o[1, :16])
    assert not torch.equal(o2[0, lens[0]:], o[0, lens[0]:])  # ... while the padded rows of the short utterance read key 0 too


@pytest.mark.parametrize("dtype,dh", [(torch.float32, 64), (torch.bfloat16, 64)])
@pytest.mark.parametrize("mask", ["none", "w3_5"])
def test_use_mask_0_ignores_the_lengths(dev, dtype, dh, mask):
    T = 65
    kw = MASKS[mask]
    out, lse = _run(dev, T, dh, dtype, mask, 0, use_mask=False)
    qkv = _operands(T, dh, dtype)
    want, wl = TO.attention_qkv(qkv.double(), B, H, T, dh, 1.0 / math.sqrt(dh), lens=_lens(T)[0], use_mask=False, want_lse=True, **kw)
    if dtype == torch.float32:
        w32 = TO.attention_qkv(qkv, B, H, T, dh, 1.0 / math.sqrt(dh), lens=None, use_mask=False, **kw)
        assert float((out - want).abs().max()) <= 4 * float((w32.double() - want).abs().max())
    else:
        fl = TO.bf16_round(TO.attention_qkv(qkv.double(), B, H, T, dh, 1.0 / math.sqrt(dh), use_mask=False, pround=TO.bf16_round, **kw))
        assert float(torch.sqrt(((out - want) ** 2).sum())) <= 2 * float(torch.sqrt(((fl - want) ** 2).sum()))
    # without a length tensor at all
    o2 = K.attn_plain_fwd(qkv.to(dev), None, B, H, T, dh, 1.0 / math.sqrt(dh), use_mask=False, causal=False, chunk_size=kw.get("chunk"),
                          history_size=kw.get("hist"))
    assert torch.equal(o2.double().cpu(), out)


def test_unsupported_head_size_launches_nothing(dev):
    T, dh = 8, 96
    qkv = torch.randn(B * T, 3 * H * dh, device=dev).to(torch.bfloat16)
    out = torch.full((B * T, H * dh), 7.0, device=dev, dtype=torch.bfloat16)
    lens = torch.tensor([8, 8, 8], dtype=torch.int32, device=dev)
    n0 = K.launch_count()
    with pytest.raises(_lib.TfasrUnsupported):
        K.attn_plain_fwd(qkv, lens, B, H, T, dh, 0.1, out=out)
    torch.cuda.synchronize()
    assert K.launch_count() == n0 and bool((out == 7.0).all())
    f = K.attn_plain_fwd(qkv.float(), lens, B, H, T, dh, 0.1)  # the f32 twin takes any multiple of 16
    assert torch.isfinite(f).all()
    with pytest.raises(_lib.TfasrUnsupported):
        K.attn_plain_fwd(torch.randn(B * T, 3 * H * 24, device=dev), lens, B, H, T, 24, 0.1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_add_pe(dev, dtype):
    Bx, T, d = 3, 37, 24
    g = torch.Generator().manual_seed(1)
    x = torch.randn(Bx, T, d, generator=g).to(dtype)
    pe = TO.sinusoid_pe(T, d, True, torch.float32).contiguous()
    lens = [0, 20, 37]
    y = K.add_pe(x.to(dev), pe.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev))
    m = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()[:, :, None]
    want = (x.float() + pe[None] * m).to(dtype)  # one f32 addition, rounded once to the storage type
    assert torch.equal(y.cpu(), want)
    y2 = K.add_pe(x.to(dev), pe.to(dev), None)
    assert torch.equal(y2.cpu(), (x.float() + pe[None]).to(dtype))
