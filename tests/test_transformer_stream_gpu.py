"""Streaming Transformer sessions on the GPU (tensorflowasr_amd/streaming.py: TransformerStreamState, transformer_encode_chunk;
csrc/stream.hip: tfasr_stream_attn_plain_fwd, tfasr_stream_add_pe) against the chunk-by-chunk float64 oracle that
tests/test_transformer_stream_oracle.py proves equal to the offline oracle of an utterance ALONE, against the recorded run of the
reference's own classes (tests/golden/transformer_wiring.npz, rows 0 and 2: the batch rows that are the utterance alone), and against the
project's own offline path.

Bars.  Kernels: tests/test_stream_gpu.py's for its attention (f32 rtol 1e-4 / atol 1e-5, bf16 2e-2 / 2e-2).  Sessions: the rules of
tests/test_transformer_gpu.py - f32 within 4 x the largest error of the oracle's own arithmetic run in float32 on the CPU, bf16 relative
error within 2 x the rounding floor (a float64 run that rounds features, weights, stored activations and probabilities to bf16), both on
the oracle's features of each utterance alone.  Every measured error and its bar goes to profiles/transformer_stream_parity.json."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tensorflowasr_amd import base_model, configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd import tokenizers as tk
from tensorflowasr_amd.schemas import PredictInput
from tensorflowasr_amd.transformer import TransformerCTC, TransformerTransducer

import stream_oracle as SO
import transformer_cases as C
import transformer_oracle as TO
import transformer_stream_oracle as TSO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = os.path.join(ROOT, "tests", "golden", "librispeech", "characters", "english.vocab")
PARITY = os.path.join(ROOT, "profiles", "transformer_stream_parity.json")
DT = [torch.float32, torch.bfloat16]
VARIANTS = {"chunked": {}, "causal": dict(use_attention_causal_mask=True), "pre": dict(norm_position="pre")}
SENTINEL = 777.0  # what a ring slot holds that no frame has been written to: a kernel that read one would show it


def _record(key, **figures):
    os.makedirs(os.path.dirname(PARITY), exist_ok=True)
    rec = {}
    if os.path.exists(PARITY):
        with open(PARITY) as f:
            rec = json.load(f)
    rec.setdefault(key, {}).update(figures)
    with open(PARITY, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


def _bar(dtype):
    return dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)


def _name(dtype):
    return "f32" if dtype == torch.float32 else "bf16"


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


def _maxerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


# =============================================================================================== 1. the attention kernel
def _case(dev, dtype, H, dh, C_, hist, seen, nvalid, seed, misalign=False):
    """random chunk + history per stream (values representable in `dtype`) -> host tensors, the rings as they stand before the launch, and
    the device arguments.  Slots no frame was written to hold SENTINEL."""
    g = torch.Generator().manual_seed(seed)
    B, HD = len(seen), H * dh

    def rnd(*shape, s=0.7):
        return (torch.randn(*shape, H, dh, generator=g) * s).to(dtype).float()

    qkv = torch.stack([rnd(B * C_), rnd(B * C_), rnd(B * C_)], 1)  # [B*C, 3, H, dh]
    kc, vc = torch.full((B, max(hist, 1), H, dh), SENTINEL)[:, :hist], torch.full((B, max(hist, 1), H, dh), SENTINEL)[:, :hist]
    hks, hvs = [], []
    for b in range(B):
        nh = min(seen[b], hist)
        hk, hv = rnd(nh), rnd(nh)  # frames seen - nh .. seen - 1 in time order
        for j in range(nh):
            kc[b, (seen[b] - nh + j) % hist], vc[b, (seen[b] - nh + j) % hist] = hk[j], hv[j]
        hks.append(hk)
        hvs.append(hv)
    flat = qkv.reshape(B * C_, 3 * HD).to(dtype)
    if misalign:  # the same rows behind one spare element: a view whose first byte is 4 (f32) or 2 (bf16) past a 16-byte boundary
        buf = torch.empty(flat.numel() + 1, dtype=dtype, device=dev)
        buf[1:] = flat.reshape(-1).to(dev)
        dq = buf[1:].view(B * C_, 3 * HD)
        assert dq.data_ptr() % 16 != 0
    else:
        dq = flat.to(dev)
    ring = lambda t: t.reshape(B, hist, HD).to(dtype).to(dev).contiguous() if hist > 0 else None
    return dict(qkv=qkv, hk=hks, hv=hvs, kc0=kc.reshape(B, hist, HD).to(dtype), vc0=vc.reshape(B, hist, HD).to(dtype), dq=dq, dkc=ring(kc), dvc=ring(vc),
                seen=_i32(seen, dev), nv=_i32(nvalid, dev))


def _check(dev, dtype, H, dh, C_, hist, seen, nvalid, seed, causal, misalign=False):
    """one launch of tfasr_stream_attn_plain_fwd: the context against the f64 oracle per stream, rows >= nvalid zero, an idle stream's
    rings bit-equal to before, the other rings exactly the chunk's rows at (seen + r) % hist and everything else untouched"""
    d = _case(dev, dtype, H, dh, C_, hist, seen, nvalid, seed, misalign)
    B, HD, scale = len(seen), H * dh, 1.0 / math.sqrt(dh)
    out = K.stream_attn_plain_fwd(d["dq"], d["dkc"], d["dvc"], d["seen"], d["nv"], B, C_, H, dh, hist, scale, causal=causal)
    torch.cuda.synchronize()
    out = out.view(B, C_, H, dh).float().cpu()
    d["worst"] = 0.0
    for b in range(B):
        n = nvalid[b]
        assert not out[b, n:].any(), b  # rows >= nvalid are zero
        if n:
            q, k, v = (d["qkv"][b * C_:b * C_ + n, i].double() for i in range(3))
            ref = TSO.attn_chunk(q, k, v, d["hk"][b].double(), d["hv"][b].double(), scale, causal)
            d["worst"] = max(d["worst"], _maxerr(out[b, :n], ref))
            np.testing.assert_allclose(out[b, :n].numpy(), ref.numpy(), **_bar(dtype), err_msg=f"stream {b}")
    if hist > 0:
        kc, vc = d["dkc"].cpu(), d["dvc"].cpu()
        rows = d["qkv"].reshape(B, C_, 3 * HD).to(dtype)
        for b in range(B):
            exp_k, exp_v = d["kc0"][b].clone(), d["vc0"][b].clone()
            for r in range(max(0, nvalid[b] - hist), nvalid[b]):
                exp_k[(seen[b] + r) % hist], exp_v[(seen[b] + r) % hist] = rows[b, r, HD:2 * HD], rows[b, r, 2 * HD:]
            assert torch.equal(kc[b], exp_k) and torch.equal(vc[b], exp_v), b  # (nvalid 0: bit-equal to before)
    return d, out


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("H,dh", [(4, 8), (4, 64), (2, 128), (2, 48)])
@pytest.mark.parametrize("dtype", DT)
def test_plain_chunk_attention_against_the_oracle(dev, dtype, H, dh, causal):
    """one batch: a fresh stream, a half-filled ring with one valid row, a ring that has wrapped, an idle stream, a partial chunk; the
    history (24) is no multiple of the chunk (16).  Head 48 does not divide the workgroup: 5 row groups and 16 idle threads."""
    d, _ = _check(dev, dtype, H, dh, 16, 24, [0, 11, 64 + 16 * 3, 37, 48], [16, 1, 16, 0, 5], 7, causal)
    _record(f"kernel_{_name(dtype)}_{H}x{dh}" + ("_causal" if causal else ""), max_abs_error=d["worst"], **_bar(dtype))


@pytest.mark.parametrize("dtype", DT)
def test_plain_chunk_attention_edges(dev, dtype):
    _check(dev, dtype, 4, 8, 4, 0, [0, 8, 12], [4, 3, 0], 3, False)  # no history at all: the rings are NULL
    _check(dev, dtype, 4, 8, 4, 0, [0, 8, 12], [4, 3, 0], 3, True)
    # fewer slots than chunk rows (hist 2 < C 4) at seen 4: both slots are read as history AND overwritten by rows 2, 3 in the same launch
    d, _ = _check(dev, dtype, 2, 8, 4, 2, [4, 0, 5], [4, 4, 3], 4, False)
    assert not (d["dkc"] == SENTINEL).any()
    _check(dev, dtype, 4, 128, 16, 64, [0, 40, 200, 77], [16, 16, 7, 0], 5, False)  # the shipped shape: chunk 16, history 64, 4 heads of 128
    _check(dev, dtype, 4, 128, 16, 64, [0, 40, 200, 77], [16, 16, 7, 0], 5, True)


@pytest.mark.parametrize("dtype", DT)
def test_plain_chunk_attention_at_the_limits_and_on_a_misaligned_view(dev, dtype):
    _check(dev, dtype, 1, 128, 32, 480, [1000, 300], [32, 17], 6, False)  # 512 keys in 16 blocks, 16 rows per thread
    _check(dev, dtype, 4, 8, 16, 24, [0, 11, 112, 37, 48], [16, 1, 16, 0, 5], 8, True, misalign=True)  # the scalar path
    _check(dev, dtype, 2, 12, 16, 24, [30, 5], [16, 9], 9, False)  # a head that is no multiple of 8: the scalar path on aligned pointers
    C_ = K.STREAM_MAX_CHUNK + 1  # beyond the limits: an error, and nothing is launched
    z, ring = torch.zeros(C_, 24, device=dev), torch.zeros(1, 4, 8, device=dev)
    i = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(K._lib.TfasrUnsupported):
        K.stream_attn_plain_fwd(z, ring, ring.clone(), i, i, 1, C_, 1, 8, 4, 1.0)
    with pytest.raises(K._lib.TfasrError, match="contiguous rows"):
        K.stream_attn_plain_fwd(z[:, :12], ring, ring.clone(), i, i, 1, C_, 1, 4, 4, 1.0)


@pytest.mark.parametrize("dtype", DT)
def test_plain_attention_equals_the_relative_kernel_with_a_zero_table(dev, dtype):
    """what the library could do before: tfasr_stream_attn_fwd fed an all-zero position table and zero biases, then tfasr_stream_kv_append"""
    H, dh, C_, hist = 4, 64, 16, 24
    seen, nvalid = [0, 11, 112, 37, 48], [16, 1, 16, 0, 5]
    B, HD, scale = len(seen), H * dh, 1.0 / math.sqrt(dh)
    d = _case(dev, dtype, H, dh, C_, hist, seen, nvalid, 11)
    kc1, vc1 = d["dkc"].clone(), d["dvc"].clone()
    zero = torch.zeros(HD, device=dev)
    pos = torch.zeros(hist + 2 * C_ - 1, HD, dtype=dtype, device=dev)
    want = K.stream_attn_fwd(d["dq"], zero, zero, pos, kc1, vc1, d["seen"], d["nv"], B, C_, H, dh, hist, scale)
    K.stream_kv_append(d["dq"], kc1, vc1, d["seen"], d["nv"], B, C_, H, dh, hist)
    got = K.stream_attn_plain_fwd(d["dq"], d["dkc"], d["dvc"], d["seen"], d["nv"], B, C_, H, dh, hist, scale)
    torch.cuda.synchronize()
    np.testing.assert_allclose(got.float().cpu().numpy(), want.float().cpu().numpy(), **_bar(dtype))
    assert torch.equal(d["dkc"], kc1) and torch.equal(d["dvc"], vc1)


# =============================================================================================== 2. the position rows
@pytest.mark.parametrize("dtype", DT)
def test_stream_add_pe(dev, dtype):
    from tensorflowasr_amd.transformer import sinusoid_table

    g = torch.Generator().manual_seed(2)
    B, C_, d, Tcap = 4, 4, 64, 40
    seen, nvalid = [0, 7, 33, 36], [4, 2, 0, 4]
    pe = torch.from_numpy(sinusoid_table(Tcap, d, True)).to(dev)
    x = torch.randn(B, C_, d, generator=g).to(dtype).to(dev)
    y = K.stream_add_pe(x, pe, _i32(seen, dev), _i32(nvalid, dev))
    # tfasr_add_pe on the same rows placed at their offsets in a [B, Tcap, d] buffer
    wide = torch.zeros(B, Tcap, d, dtype=dtype, device=dev)
    for b in range(B):
        wide[b, seen[b]:seen[b] + C_] = x[b]
    want = K.add_pe(wide, pe)
    torch.cuda.synchronize()
    for b in range(B):
        n = nvalid[b]
        assert torch.equal(y[b, :n], want[b, seen[b]:seen[b] + n]), b  # bit-equal
        assert torch.equal(y[b, n:], x[b, n:]), b  # rows that are not valid: unchanged
    # a table that ends too early: the rows past it are NaN, the table is not read past its end, the launch completes
    y = K.stream_add_pe(x, pe[:38].contiguous(), _i32(seen, dev), _i32(nvalid, dev))
    torch.cuda.synchronize()
    assert torch.equal(y[:3], K.stream_add_pe(x, pe, _i32(seen, dev), _i32(nvalid, dev))[:3])
    assert torch.equal(y[3, :2], want[3, 36:38]) and bool(torch.isnan(y[3, 2:].float()).all())
    # a width that is no multiple of 8 (the scalar path): f32 add, one rounding
    x2 = torch.randn(2, 3, 20, generator=g).to(dtype).to(dev)
    pe2 = torch.randn(9, 20, generator=g).to(dev)
    y2 = K.stream_add_pe(x2, pe2, _i32([1, 6], dev), _i32([3, 2], dev))
    exp = x2.clone()
    exp[0] = (x2[0].float() + pe2[1:4]).to(dtype)
    exp[1, :2] = (x2[1, :2].float() + pe2[6:8]).to(dtype)
    assert torch.equal(y2, exp)
    assert K.stream_add_pe(x, pe, _i32(seen, dev), _i32(nvalid, dev), y=x) is x  # in place


# =============================================================================================== 3. models and references
def build(dev, variant="chunked", dtype=torch.float32, cls=TransformerCTC, head="ctc"):
    cfg = C.tiny_config("chunked", head=head, **VARIANTS[variant])
    model = cls(cfg, dev, dtype=dtype, seed=3)
    model.ps.import_keras(C.make_weights(cfg))
    model.tokenizer = tk.get({"type": "characters", "blank_index": 0, "vocabulary": VOCAB})
    return model


_REFS = {}


def _alone(cfg, W, own):
    """per utterance ALONE, on its own features: the f64 oracle's frames, its float32 run, its bf16-rounded run"""
    enc = [TSO.offline_alone(f, W, cfg) for f in own]
    enc32 = [TSO.offline_alone(f, W, cfg, dtype=torch.float32) for f in own]
    floor = [TSO.offline_alone(f, W, cfg, rounder=TO.bf16_round, wround=TO.bf16_round) for f in own]
    return dict(cfg=cfg, W=W, own=own, enc=enc, enc32=enc32, floor=floor)


def reference(variant):
    """the tiny cases of tests/transformer_cases.py, each utterance alone; computed once on the CPU and shared"""
    if variant not in _REFS:
        cfg = C.tiny_config("chunked", **VARIANTS[variant])
        W, sig = C.make_weights(cfg), C.audio()
        own = [C.features(sig[b:b + 1, :n], cfg)[0] for b, n in enumerate(C.SAMPLES)]
        ref = _alone(cfg, W, own)
        lg = [TO.logits(e, W) for e in ref["enc"]]
        lg32 = [TO.logits(e, W, torch.float32) for e in ref["enc32"]]
        top2 = [torch.topk(l, 2, -1).values for l in lg]
        ref.update(sigs=[sig[b, :n] for b, n in enumerate(C.SAMPLES)], tokens=[C.collapse(l.numpy(), l.shape[0]) for l in lg],
                   margin=min(float((t[:, 0] - t[:, 1]).min()) for t in top2), logit_err32=max(_maxerr(a, b) for a, b in zip(lg32, lg)))
        _REFS[variant] = ref
    return _REFS[variant]


def _encode_streams(model, own, precision):
    """the oracle's features of B utterances through encode_chunk as B streams of ONE state: ragged lengths, stream b idle in step
    b + 1 (so the streams stop moving in step), a partial last chunk each -> the valid frames per stream, the launches of a full step"""
    B, n0 = len(own), 4 * model.cfg.chunk_size
    state = model.stream_state(B, precision=precision)
    dt, dev = state.model.dtype, model.device
    pos, outs, step = [0] * B, [[] for _ in range(B)], 0
    while any(pos[b] < own[b].shape[0] for b in range(B)):
        take = [0 if step == b + 1 else min(n0, own[b].shape[0] - pos[b]) for b in range(B)]
        step += 1
        if max(take) == 0:
            continue
        feats = torch.zeros(B, max(take), own[0].shape[1], dtype=torch.float64)
        for b in range(B):
            feats[b, :take[b]] = own[b][pos[b]:pos[b] + take[b]]
            pos[b] += take[b]
        enc, nvalid = model.encode_chunk(state, feats.to(dt).to(dev).contiguous(), take)
        nv = nvalid.tolist()
        assert nv == [TO.reduced_length(t) for t in take]
        for b in range(B):
            outs[b].append(enc[b, :nv[b]].float().cpu())
    assert state.seen.tolist() == [TO.reduced_length(f.shape[0]) for f in own] == state.host_seen
    return [torch.cat(o, 0) for o in outs]


def _session_bars(key, got, ref, dtype):
    """the two rules of tests/test_transformer_gpu.py over all streams of the session"""
    cat = lambda xs: np.concatenate([np.asarray(x, np.float64) for x in xs])
    for g, e in zip(got, ref["enc"]):
        assert g.shape == e.shape
    if dtype == torch.float32:
        err, bar = _maxerr(cat(got), cat(ref["enc"])), 4 * _maxerr(cat(ref["enc32"]), cat(ref["enc"]))
        print(f"{key}: f32 session against the f64 oracle alone: {err:.3e} (bar {bar:.3e})")
        _record(key, f32_error=err, f32_bar=bar)
        assert err <= bar
    else:
        err, floor = _rel(cat(got), cat(ref["enc"])), _rel(cat(ref["floor"]), cat(ref["enc"]))
        print(f"{key}: bf16 session relative error {err:.3e}, rounding floor {floor:.3e}")
        _record(key, bf16_rel_error=err, bf16_rounding_floor=floor, allowed=2 * floor)
        assert floor > 0 and err <= 2 * floor


@pytest.mark.parametrize("variant,dtype", [("chunked", torch.float32), ("chunked", torch.bfloat16), ("pre", torch.float32), ("causal", torch.float32)])
def test_encoder_session_on_the_oracles_features(dev, variant, dtype):
    ref = reference(variant)
    model = build(dev, variant, dtype)
    got = _encode_streams(model, ref["own"], _name(dtype))
    _session_bars(f"session_{variant}_{_name(dtype)}", got, ref, dtype)


def test_streams_0_and_2_against_the_recorded_reference_run(dev, tmp_path):
    """rows 0 and 2 of the reference's padded batch are those utterances alone (tests/test_transformer_stream_oracle.py): reference-made
    expected values for a session.  Bar: the recorded run's own (4 x the f32 oracle's error + the fixture's distance from the f64 oracle)
    plus the oracle's batch-against-alone distance on that row."""
    with np.load(C.WIRING) as z:
        wiring = {k: z[k] for k in z.files}
    path = os.path.join(tmp_path, "wiring.npz")
    with open(path, "wb") as f:
        np.savez(f, **{k[2:]: v for k, v in wiring.items() if k.startswith("w|")})
    model = TransformerCTC(C.tiny_config("chunked"), dev, dtype=torch.float32, seed=99)
    model.load_weights(path)
    ref, batch = reference("chunked"), C.reference("chunked")
    assert np.array_equal(wiring["feats"], batch["feats"].float().numpy())
    got = _encode_streams(model, ref["own"], "f32")
    want = wiring["chunked|encoder"]
    for b in (0, 2):
        n = C.ELEN[b]
        bar = (4 * _maxerr(batch["enc32"], batch["enc"]) + _maxerr(want[b, :n], batch["enc"][b, :n])
               + _maxerr(batch["enc"][b, :n], ref["enc"][b]))
        err = _maxerr(got[b], want[b, :n])
        print(f"stream {b} against the recorded reference run: {err:.3e} (bar {bar:.3e})")
        _record(f"wiring_stream_{b}", error=err, bar=bar)
        assert err <= bar


_SHIPPED = {}


def _shipped(dev, dtype):
    """base-streaming.yml.j2's attention shape (chunk 16, history 64, 4 heads of 128, d 512) with one block and 32 subsampling filters;
    1.0 / 2.6 / 4.1 s of seeded noise: 25 / 65 / 103 encoder frames, so that the 64-slot ring wraps"""
    with open(C.CONFIG_FIXTURE) as f:
        fx = json.load(f)["base-streaming"]
    conf = dict(fx["config"], encoder_num_blocks=1, vocab_size=29)
    conf["encoder_subsampling"] = dict(conf["encoder_subsampling"], filters=[32, 32])
    model = base_model.model_from_config({"class_name": fx["class_name"], "config": conf}, device=dev, dtype=dtype)
    cfg = model.cfg
    assert (cfg.chunk_size, cfg.history_size, cfg.num_heads, cfg.head_size, cfg.num_blocks, cfg.sub_filters) == (16, 64, 4, 128, 1, [32, 32])
    if "ref" not in _SHIPPED:
        W = C.make_weights(cfg)
        own = [C.features(s[None], cfg)[0] for s in SO.noise(21, [1.0, 2.6, 4.1])]
        _SHIPPED["ref"] = _alone(cfg, W, own)
    model.ps.import_keras(_SHIPPED["ref"]["W"])
    return model, _SHIPPED["ref"]


@pytest.mark.parametrize("dtype", DT)
def test_encoder_session_at_the_shipped_attention_shape(dev, dtype):
    model, ref = _shipped(dev, dtype)
    assert [e.shape[0] for e in ref["enc"]] == [25, 65, 103]
    got = _encode_streams(model, ref["own"], _name(dtype))
    _session_bars(f"shipped_shape_{_name(dtype)}", got, ref, dtype)


# =============================================================================================== 4. sessions from the audio
def _feed(rec, sigs, pieces):
    """all streams fed the next of `pieces` samples per call (cycling; ragged ends), then finish -> (tokens, encoder frames, frame counts)"""
    B = len(sigs)
    rec.encoded_log = []
    toks = [[] for _ in range(B)]

    def take(out):
        for b in range(B):
            toks[b] += out.tokens[b, :int(out.tokens_length[b])].tolist()
        return out.frames.tolist()

    n, p0, k = max(len(s) for s in sigs), 0, 0
    while p0 < n:
        piece = pieces[k % len(pieces)]
        x = np.zeros((B, piece), np.float32)
        lens = []
        for b, s in enumerate(sigs):
            seg = s[p0:p0 + piece]
            x[b, :len(seg)] = seg
            lens.append(len(seg))
        take(rec.accept(torch.from_numpy(x), lens))
        p0, k = p0 + piece, k + 1
    frames = take(rec.finish())
    enc = [torch.cat([e[b, :nv[b]] for e, nv in rec.encoded_log] + [rec.encoded_log[0][0][b, :0]], 0).float().cpu() for b in range(B)]
    return toks, enc, frames


def _tokens_of(out):
    return [v for v in out.tokens[0].tolist() if v != 0]


def _recognize_alone(model, sig, **kw):
    return _tokens_of(model.recognize(PredictInput(torch.from_numpy(np.ascontiguousarray(sig))[None], torch.tensor([len(sig)])), **kw))


@pytest.mark.parametrize("variant", ["chunked", "causal"])
def test_tokens_equal_recognize_alone_and_the_oracle(dev, variant):
    """f32 session from the audio: each stream's concatenated output is model.recognize of that utterance alone and the f64 oracle's
    greedy tokens of it alone.  Near-ties are excluded by the input, not by the comparison: the oracle's smallest top-two margin must be
    100 x the float32 logit error."""
    ref = reference(variant)
    print(f"{variant}: smallest top-two margin of the oracle alone {ref['margin']:.3e}, f32 logit error {ref['logit_err32']:.3e}")
    _record(f"tokens_{variant}", margin=ref["margin"], f32_logit_error=ref["logit_err32"])
    assert ref["margin"] > 100 * ref["logit_err32"] and all(len(t) > 3 for t in ref["tokens"])
    model = build(dev, variant)
    toks, enc, frames = _feed(model.stream(3), ref["sigs"], [4000])
    assert frames == C.ELEN
    for b in range(3):
        assert toks[b] == ref["tokens"][b], b
        assert toks[b] == _recognize_alone(model, ref["sigs"][b]), b
    err, bar = max(_maxerr(e, r) for e, r in zip(enc, ref["enc"])), 4 * max(_maxerr(a, r) for a, r in zip(ref["enc32"], ref["enc"]))
    _record(f"tokens_{variant}", frames_error_from_audio=err, frames_bar_on_the_oracles_features=bar)


def test_arrival_does_not_matter_and_a_reused_slot_is_a_fresh_stream(dev):
    ref = reference("chunked")
    model, sigs = build(dev), ref["sigs"]
    base_t, base_e, _ = _feed(model.stream(3), sigs, [20000])  # each utterance whole
    assert base_t == ref["tokens"]
    for pieces in ([1600], [733, 160, 4001, 57]):  # 100 ms at a time; uneven pieces
        t, e, _ = _feed(model.stream(3), sigs, pieces)
        assert t == base_t, pieces
        for b in range(3):
            assert torch.equal(e[b], base_e[b]), (pieces, b)
    # slot 1 takes utterance 0, finishes, is reset and takes utterance 1 while slot 0 is in the middle of utterance 2
    rec = model.stream(3)
    rec.encoded_log = []
    a, first, second = sigs[2], sigs[0], sigs[1]
    x = np.zeros((3, 6000), np.float32)
    x[0], x[1, :len(first)] = a[:6000], first
    out = rec.accept(torch.from_numpy(x), [6000, len(first), 0])
    t1 = out.tokens[1, :int(out.tokens_length[1])].tolist()
    out = rec.finish(rows=[1])
    t1 += out.tokens[1, :int(out.tokens_length[1])].tolist()
    assert t1 == base_t[0]
    with pytest.raises(RuntimeError, match="finished"):
        rec.accept(torch.from_numpy(np.zeros((3, 160), np.float32)), [0, 160, 0])
    rec.reset(rows=[1])
    mark = len(rec.encoded_log)
    x = np.zeros((3, len(second)), np.float32)
    x[0, :len(a) - 6000], x[1] = a[6000:], second
    out = rec.accept(torch.from_numpy(x), [len(a) - 6000, len(second), 0])
    t2 = out.tokens[1, :int(out.tokens_length[1])].tolist()
    out = rec.finish()
    t2 += out.tokens[1, :int(out.tokens_length[1])].tolist()
    got0 = torch.cat([e[0, :nv[0]] for e, nv in rec.encoded_log], 0).float().cpu()
    got1a = torch.cat([e[1, :nv[1]] for e, nv in rec.encoded_log[:mark]], 0).float().cpu()
    got1b = torch.cat([e[1, :nv[1]] for e, nv in rec.encoded_log[mark:]], 0).float().cpu()
    assert torch.equal(got0, base_e[2])  # the stream beside the reset one: bit-equal
    assert torch.equal(got1a, base_e[0]) and torch.equal(got1b, base_e[1]) and t2 == base_t[1]  # the reused slot: a fresh stream
    assert out.frames.tolist() == [C.ELEN[2], C.ELEN[1], 0]


def test_transducer_session_equals_recognize_alone(dev):
    model = build(dev, cls=TransformerTransducer, head="rnnt")
    sigs = reference("chunked")["sigs"]
    toks, _, frames = _feed(model.stream(3), sigs, [4000])
    assert frames == C.ELEN and sum(len(t) for t in toks) > 0
    for b in range(3):
        assert toks[b] == _recognize_alone(model, sigs[b]), b
    # the encoder state rides through the predict schemas and back into a session
    rec = model.stream(1)
    rec.accept(torch.from_numpy(sigs[2][:5000])[None])
    st = rec.encoder_state()
    out = model.recognize(PredictInput(torch.from_numpy(sigs[0])[None], torch.tensor([len(sigs[0])]), previous_encoder_states=st))
    assert out.next_encoder_states is st


def test_ctc_beam_session_equals_the_one_shot_search_on_its_own_frames(dev):
    model = build(dev)
    sigs = reference("chunked")["sigs"]
    B, W = 3, 4
    rec = model.stream(B, beam_width=W)
    toks, _, _ = _feed(rec, sigs, [733])
    per = [torch.cat([e[b, :nv[b]] for e, nv in rec.encoded_log], 0) for b in range(B)]
    lens = [int(p.shape[0]) for p in per]
    enc = torch.zeros(B, max(lens), per[0].shape[1], dtype=per[0].dtype, device=dev)
    for b, p in enumerate(per):
        enc[b, :lens[b]] = p
    logits = K.matmul(enc.float().reshape(-1, enc.shape[2]).contiguous(), model.ps.p2d("dec/logits/w"), bias=model.ps.p("dec/logits/b"))
    want = K.ctc_beam_search_device(logits.view(B, enc.shape[1], -1), lens, W, W, None)
    for name, a, b in zip(("tokens", "lengths", "log_prob"), rec.hypotheses(W), want):
        assert torch.equal(a.cpu(), b.cpu()), name
    wt, wn = want[0].cpu(), want[1].cpu()
    assert lens == C.ELEN and sum(len(t) for t in toks) > 0
    for b in range(B):
        assert toks[b] == wt[b, 0, :int(wn[b, 0])].tolist(), b


def test_encoder_state_round_trip(dev):
    model, sigs = build(dev), reference("chunked")["sigs"]
    rec = model.stream(1)
    rec.encoded_log = []
    rec.accept(torch.from_numpy(sigs[2][:6400 + 240])[None])  # 2 chunks and the 240 samples the next frame still needs
    st = rec.encoder_state()
    assert len(st) == 3 + 2 * model.cfg.num_blocks and st[0].tolist() == [8]
    rec2 = model.stream(1)
    rec2.set_encoder_state(st)
    for a, b in zip(rec2.encoder_state(), st):
        assert torch.equal(a, b)
    assert rec2.state.host_seen == [8]
    # the copy is a copy, and a session that continues from it computes what the first one computes
    feats = torch.from_numpy(reference("chunked")["own"][2][32:48].numpy()).float().to(dev)[None].contiguous()
    e1, _ = model.encode_chunk(rec.state, feats, [16])
    assert st[0].tolist() == [8] and rec.state.seen.tolist() == [12]
    e2, _ = model.encode_chunk(rec2.state, feats, [16])
    assert torch.equal(e1, e2)
    with pytest.raises(ValueError, match="another model"):
        rec2.set_encoder_state(st[:-1])


def test_position_table_grows_past_its_first_size(dev):
    """a stream that runs past the table's first 256 rows: the rows behind the growth are the rows a table made in one piece has"""
    model = build(dev)
    state = model.stream_state(2)
    assert state.pe.shape[0] == 256
    state.seen += _i32([254, 0], dev)
    state.host_seen = [254, 0]
    feats = torch.zeros(2, 16, 16, device=dev)
    enc, nv = model.encode_chunk(state, feats, [16, 16])  # stream 0: positions 254 .. 257
    torch.cuda.synchronize()
    assert state.pe.shape[0] == 512 and state.host_seen == [258, 4] and bool(torch.isfinite(enc).all())
    from tensorflowasr_amd.transformer import sinusoid_table

    assert torch.equal(state.pe.cpu(), torch.from_numpy(sinusoid_table(512, 64, True)))
    assert torch.equal(state.pe[:256].cpu(), torch.from_numpy(sinusoid_table(256, 64, True)))


def test_latency_in_samples(dev):
    """encoder frame C (c + 1) - 1 needs 640 C (c + 1) + 240 samples and appears not one sample earlier; after finish the count is
    ceil(ceil(ceil(n / 160) / 2) / 2)"""
    model = build(dev)
    C_ = model.cfg.chunk_size
    for c in (0, 1, 3):
        need = 640 * C_ * (c + 1) + 240
        rec = model.stream(1)
        assert rec.accept(torch.zeros(1, need - 1)).frames.tolist() == [C_ * c]
        assert rec.accept(torch.ones(1, 1) * 0.1).frames.tolist() == [C_ * (c + 1)]
    for n in (1, 159, 160, 161, 640 * C_ + 239, 640 * C_ + 240, 5000, 12345):
        rec = model.stream(1)
        rec.accept(torch.zeros(1, n))
        assert rec.finish().frames.tolist() == [TO.reduced_length(-(-n // 160))], n


def test_refusals_at_session_creation(dev):
    def tiny(**over):
        return TransformerCTC(C.tiny_config("full", **over), dev, dtype=torch.float32, seed=0)

    for model, reason in ((tiny(), "chunk_size is None"), (tiny(chunk_size=4, history_size=8, use_attention_auto_mask=False), "use_attention_auto_mask"),
                          (tiny(chunk_size=4, history_size=-1), "unlimited history"),
                          (tiny(chunk_size=K.STREAM_MAX_CHUNK + 1, history_size=8), "limits"),
                          (tiny(chunk_size=16, history_size=K.STREAM_MAX_KEYS), "limits")):
        for call in (lambda: model.stream(), lambda: model.stream_state(2), lambda: model.encode_chunk(None, None, None)):
            with pytest.raises(NotImplementedError, match="inference only.*" + reason):
                call()
    model = build(dev)
    with pytest.raises(ValueError, match="chunk_frames"):
        from tensorflowasr_amd.streaming import StreamingRecognizer

        StreamingRecognizer(model, chunk_frames=32)
    with pytest.raises(ValueError, match="beam_width"):
        model.stream(beam_width=65)
    rec = model.stream(1)
    rec.accept(torch.zeros(1, 4000))
    rec.finish()
    with pytest.raises(RuntimeError, match="finished"):
        rec.accept(torch.zeros(1, 160))
    rec.reset()
    assert rec.accept(torch.zeros(1, 4000)).frames.tolist() == [4]
    assert isinstance(configs.transformer(streaming=True), configs.TransformerConfig)
