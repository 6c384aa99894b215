"""The float64 Transformer oracle (tests/transformer_oracle.py) pinned on the CPU: its attention against the literal [B, T, T] mask +
masked_fill definition, the position table against compute_sinusoid_position_encoding restated, the whole oracle against
tests/golden/transformer_wiring.npz (recorded from the reference's OWN TransformerEncoder + TransformerDecoder over
oracle/keras_shim.reference_runtime()) and, where the reference tree is present, against a live run of those classes - all rows, padded
ones included, which is what pins in which blocks the query mask exists (transformer_oracle.query_masked)."""
import math

import numpy as np
import pytest
import torch

from tensorflowasr_amd import checkpoint
from tensorflowasr_amd.transformer import sinusoid_table

import transformer_cases as C
import transformer_oracle as TO

MASKS = [dict(), dict(causal=True), dict(chunk=16, hist=64), dict(chunk=3, hist=5), dict(chunk=4, hist=0), dict(chunk=16, hist=-1),
         dict(chunk=3, hist=5, causal=True)]


def _direct(q, k, v, scale, lens, use_mask, causal=False, chunk=None, hist=None):
    """per row, with the explicit boolean mask and masked_fill(-1e9): multihead_attention.py:146-213 + general.py:25-41"""
    B, H, T, dh = q.shape
    mask = torch.ones(B, T, T, dtype=torch.bool)
    if use_mask:
        mask &= (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])[:, :, None]  # query_mask[:, :, None]; keys are not masked
    if causal:
        mask &= torch.tril(torch.ones(T, T, dtype=torch.bool))[None]
    if chunk:
        stream = torch.zeros(T, T, dtype=torch.bool)
        h = T if hist < 0 else hist
        for i in range(T):
            idx = (i // chunk) * chunk
            stream[i, max(0, idx - h):min(T, idx + chunk)] = True
        mask &= stream[None]
    out = torch.zeros_like(q)
    probs = torch.zeros(B, H, T, T, dtype=q.dtype)
    for b in range(B):
        for h_ in range(H):
            for i in range(T):
                s = (q[b, h_, i] * scale) @ k[b, h_].T
                s = torch.where(mask[b, i], s, torch.full_like(s, -1e9))
                p = torch.exp(s - torch.logsumexp(s, -1))
                probs[b, h_, i] = p
                out[b, h_, i] = p @ v[b, h_]
    return out, probs


@pytest.mark.parametrize("kw", MASKS)
@pytest.mark.parametrize("use_mask", [True, False])
def test_attention_against_the_masked_fill_definition(kw, use_mask):
    g = torch.Generator().manual_seed(3)
    B, H, T, dh = 3, 2, 21, 8
    q, k, v = (torch.randn(B, H, T, dh, generator=g).double() for _ in range(3))
    lens = [0, 13, 21]
    got, lse = TO.attention(q, k, v, 0.35, lens=lens, use_mask=use_mask, want_lse=True, **kw)
    want, probs = _direct(q, k, v, 0.35, lens, use_mask, **kw)
    # A padded row of the literal form is softmax(-1e9 ...): its logsumexp is -1e9 + ln T rounded at |1e9|, whose spacing in float64 is
    # 2^-23 = 1.2e-7 - so the literal form itself carries a relative error of up to that on such a row, and no more anywhere else.
    PADDED = dict(rtol=2.4e-7, atol=0)
    for b, n in enumerate(lens):
        for i in range(T):
            lo, hi = TO.visible(i, T, kw.get("causal", False), kw.get("chunk"), kw.get("hist"))
            if use_mask and i >= n:  # a padded row: uniform over ALL T keys, with and without the streaming / causal mask
                np.testing.assert_allclose(probs[b, :, i].numpy(), np.full((H, T), 1.0 / T), **PADDED)
                np.testing.assert_allclose(got[b, :, i].numpy(), v[b].mean(1).numpy(), rtol=1e-12, atol=1e-14)
                np.testing.assert_allclose(got[b, :, i].numpy(), want[b, :, i].numpy(), rtol=0, atol=2.4e-7 * float(v[b].abs().mean(1).max()))
                assert float(lse[b, 0, i]) == math.log(T)
            else:  # a valid row: exactly zero outside its window
                np.testing.assert_allclose(got[b, :, i].numpy(), want[b, :, i].numpy(), rtol=1e-12, atol=1e-13)
                assert not probs[b, :, i, :lo].any() and not probs[b, :, i, hi:].any() and (probs[b, :, i, lo:hi] > 0).all()
                s = (q[b, :, i, None, :] * 0.35 * k[b, :, lo:hi]).sum(-1)
                np.testing.assert_allclose(lse[b, :, i].numpy(), torch.logsumexp(s, -1).numpy(), rtol=1e-12)
    # the kernel's layout is the same function
    qkv = torch.cat([t.permute(0, 2, 1, 3).reshape(B * T, H * dh) for t in (q, k, v)], 1)
    flat = TO.attention_qkv(qkv, B, H, T, dh, 0.35, lens=lens, use_mask=use_mask, **kw)
    assert torch.equal(flat, got.permute(0, 2, 1, 3).reshape(B * T, H * dh))


@pytest.mark.parametrize("interleave", [True, False])
def test_position_table_against_the_definition(interleave):
    T, d = 37, 24
    want = np.zeros((T, d))
    for t in range(T):
        for c in range(d):
            if interleave:  # timescale min_freq ** (2 (c // 2) / d); even columns sine, odd columns cosine
                ang = t * (1.0 / 10000.0) ** (2 * (c // 2) / d)
                want[t, c] = math.cos(ang) if c % 2 else math.sin(ang)
            else:           # timescales min_freq ** (2 j / d), j < d / 2; [sin | cos]
                ang = t * (1.0 / 10000.0) ** (2 * (c % (d // 2)) / d)
                want[t, c] = math.sin(ang) if c < d // 2 else math.cos(ang)
    np.testing.assert_allclose(TO.sinusoid_pe(T, d, interleave).numpy(), want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(sinusoid_table(T, d, interleave), want, rtol=0, atol=2e-5)  # the model's f32 table (angles up to T in f32)
    x = torch.zeros(2, T, d, dtype=torch.float64)
    y = TO.add_pe(x, [5, T], interleave)
    assert not y[0, 5:].any() and np.allclose(y[0, :5].numpy(), want[:5]) and np.allclose(y[1].numpy(), want)


def test_query_mask_reaches_block_0_only_under_post_norm():
    post, pre = C.tiny_config("full"), C.tiny_config("full", norm_position="pre")
    assert [TO.query_masked(post, i) for i in range(3)] == [True, False, False]
    assert [TO.query_masked(pre, i) for i in range(3)] == [True, True, True]
    assert TO.mask_args(C.tiny_config("chunked"), 1) == dict(use_mask=False, causal=False, chunk=4, hist=8)
    assert TO.mask_args(C.tiny_config("full", use_attention_auto_mask=False), 0) == dict(use_mask=False, causal=False, chunk=None, hist=None)


@pytest.fixture(scope="module")
def wiring():
    with np.load(C.WIRING) as z:
        return {k: z[k] for k in z.files}


def _weights_from(wiring, cfg):
    arrays = {k[2:].replace("|", "/"): v for k, v in wiring.items() if k.startswith("w|")}
    template = C.make_weights(cfg)
    got = checkpoint.from_keras(arrays, template, path_fn=checkpoint.transformer_keras_path)
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in got.items()}


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_whole_oracle_against_the_recorded_reference_run(wiring, setting):
    """every row, padded ones included.  The reference run (the shim) computes in float64 and stores float32 between layers."""
    cfg = C.tiny_config(setting)
    W = _weights_from(wiring, cfg)
    for k, v in C.make_weights(cfg).items():  # the fixture's weights ARE the cases' weights under the reference's names and layouts
        assert torch.equal(W[k], v), k
    flen = wiring["flen"].tolist()
    enc, elen = TO.encoder(torch.from_numpy(wiring["feats"]).double(), flen, cfg, W)
    assert elen == wiring[f"{setting}|lengths"].tolist() == C.ELEN
    np.testing.assert_allclose(enc.numpy(), wiring[f"{setting}|encoder"], rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(TO.logits(enc, W).numpy(), wiring[f"{setting}|logits"], rtol=1e-5, atol=1e-3)  # logits of O(1e2): f32 storage
    # padded rows are live: with the query mask in every block (what post-norm does NOT do) the recorded padded rows are missed
    other, _ = TO.encoder(torch.from_numpy(wiring["feats"]).double(), flen, C.tiny_config(setting, norm_position="pre"), W)
    assert not np.allclose(other[0, elen[0]:].numpy(), wiring[f"{setting}|encoder"][0, elen[0]:], rtol=1e-2, atol=1e-2)


def test_fixture_is_no_larger_than_the_other_wiring_files():
    import os

    assert os.path.getsize(C.WIRING) <= 816659  # tests/golden/wiring_conformer.npz


@pytest.mark.parametrize("setting", list(C.SETTINGS))
def test_the_chosen_seed_meets_the_conditions_on_the_input(setting):
    """tests/test_transformer_gpu.py compares greedy tokens with no frame and no utterance excluded: on every valid frame the oracle's
    top-two logit margin is at least 100 times the f32 logit error (the oracle's own arithmetic in f32 against f64), and every utterance
    says more than three tokens"""
    ref = C.reference(setting)
    assert ref["elen"] == C.ELEN and all(len(t) > 3 for t in ref["tokens"])
    print(f"{setting}: margin {ref['margin']:.3e}, f32 logit error {ref['logit_err32']:.3e}")
    assert ref["margin"] >= 100 * ref["logit_err32"]


@pytest.mark.skipif(not C.have_reference(), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("setting,over", [("full", {}), ("chunked", {}), ("full", dict(norm_position="pre", residual_factor=0.5, interleave_relpe=False)),
                                          ("chunked", dict(use_attention_causal_mask=True, sub_norm="none")),
                                          ("full", dict(use_attention_auto_mask=False))])
def test_oracle_against_a_live_run_of_the_references_classes(setting, over):
    cfg = C.tiny_config(setting, **over)
    ref = C.reference(setting, cfg=cfg)
    out, out_len, lg, arrays = C.reference_run(cfg, ref["W"], ref["feats"].float().numpy(), ref["flen"])
    assert out_len == ref["elen"] == C.ELEN
    assert "encoder/block_1/mhsa/attention_output/kernel" in arrays and arrays["encoder/block_0/mhsa/query/kernel"].shape == (64, 2, 64)
    np.testing.assert_allclose(out, ref["enc"].numpy(), rtol=1e-5, atol=1e-5)  # every row of every utterance
    np.testing.assert_allclose(lg, ref["logits"].numpy(), rtol=1e-5, atol=1e-3)
