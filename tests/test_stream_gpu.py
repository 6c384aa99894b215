"""Streaming recognition on the GPU (tensorflowasr_amd/streaming.py, csrc/stream.hip) against the chunked oracle that
tests/test_stream_oracle.py proves equal to the offline oracle, against the reference-made golden, and against the project's own
offline path (model.encode / model.recognize of each utterance ALONE)."""
import math

import numpy as np
import pytest
import torch

from oracle import conformer_ref as R
from tensorflowasr_amd import configs
from tensorflowasr_amd import kernels as K
from tensorflowasr_amd.conformer import ConformerTransducer
from tensorflowasr_amd.contextnet import ContextNetTransducer
from tensorflowasr_amd.ctc_model import ConformerCTC
from tensorflowasr_amd.schemas import PredictInput

import stream_oracle as SO

pytestmark = pytest.mark.gpu
DT = [torch.float32, torch.bfloat16]
F32_BAR, BF16_BAR = 2e-3, 3.2e-2  # tests/test_reference_wiring_gpu.py, this very model


def tol(dtype, f32=(1e-5, 1e-5), bf16=(2e-2, 2e-2)):  # tests/test_ops_gpu.py
    return dict(rtol=f32[0], atol=f32[1]) if dtype == torch.float32 else dict(rtol=bf16[0], atol=bf16[1])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def _i32(x, dev):
    return torch.tensor(x, dtype=torch.int32, device=dev)


# =============================================================================================== 1. kernels, one at a time
def _attn_case(dev, dtype, H, dh, dh_log, C, hist, seen, nvalid, seed):
    """random chunk + history per stream -> (device context, oracle context per stream, rings before, device args)"""
    g = torch.Generator().manual_seed(seed)
    B, HD = len(seen), H * dh
    pad = torch.zeros(dh)
    pad[:dh_log] = 1.0

    def rnd(*shape, s=0.7):
        return ((torch.randn(*shape, H, dh, generator=g) * s) * pad).to(dtype).float()

    qkv = torch.stack([rnd(B * C), rnd(B * C), rnd(B * C)], 1)  # [B*C, 3, H, dh]
    u, v = (torch.randn(H, dh, generator=g) * 0.3) * pad, (torch.randn(H, dh, generator=g) * 0.3) * pad
    pos = rnd(hist + 2 * C - 1)
    scale = 1.0 / math.sqrt(dh_log)
    kc, vc = torch.zeros(B, max(hist, 1), H, dh), torch.zeros(B, max(hist, 1), H, dh)
    kc, vc = kc[:, :hist], vc[:, :hist]
    refs = []
    for b in range(B):
        nh = min(seen[b], hist)
        hk, hv = rnd(nh), rnd(nh)  # frames seen - nh .. seen - 1 in time order
        for j in range(nh):
            kc[b, (seen[b] - nh + j) % hist], vc[b, (seen[b] - nh + j) % hist] = hk[j], hv[j]
        n = nvalid[b]
        q, k, vv = (qkv[b * C:b * C + n, i].double() for i in range(3))
        ref = torch.zeros(C, H, dh, dtype=torch.float64)
        if n:
            ref[:n] = SO.attn_chunk(q, k, vv, hk.double(), hv.double(), pos.double(), u.double(), v.double(), hist, C, scale)
        refs.append(ref)
    d = dict(qkv=qkv.reshape(B * C, 3 * HD).to(dev).to(dtype), u=u.reshape(-1).to(dev), v=v.reshape(-1).to(dev),
             pos=pos.reshape(-1, HD).to(dev).to(dtype), kc=kc.reshape(B, hist, HD).to(dev).to(dtype).contiguous(),
             vc=vc.reshape(B, hist, HD).to(dev).to(dtype).contiguous(), seen=_i32(seen, dev), nv=_i32(nvalid, dev))
    out = K.stream_attn_fwd(d["qkv"], d["u"], d["v"], d["pos"], d["kc"], d["vc"], d["seen"], d["nv"], B, C, H, dh, hist, scale)
    return out.view(B, C, H, dh), torch.stack(refs), d


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("H,dh,dh_log", [(4, 8, 8), (4, 64, 36)])
def test_chunk_attention_against_the_oracle(dev, dtype, H, dh, dh_log):
    """one batch: a fresh stream, a half-filled ring with one valid row, a ring that has wrapped, an idle stream, a partial chunk; streams at
    different `seen`.  bf16 bar of test_relattn_fused_forward, f32 1e-4 / 1e-5."""
    C, hist = 16, 24
    seen, nvalid = [0, 11, 64 + 16 * 3, 37, 48], [C, 1, C, 0, 5]
    out, ref, d = _attn_case(dev, dtype, H, dh, dh_log, C, hist, seen, nvalid, 7)
    kc0, vc0 = d["kc"].clone(), d["vc"].clone()
    K.stream_kv_append(d["qkv"], d["kc"], d["vc"], d["seen"], d["nv"], len(seen), C, H, dh, hist)
    torch.cuda.synchronize()
    bar = dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), **bar)
    assert not out[3].any() and not out[1, 1:].any() and not out[4, 5:].any()  # rows >= nvalid are zero
    if dh_log < dh:
        assert not out[..., dh_log:].any()  # the padding of a head stored wider stays zero
    # the idle stream's rings are untouched, bit for bit; the others hold the chunk's rows at (seen + r) % hist
    assert torch.equal(d["kc"][3], kc0[3]) and torch.equal(d["vc"][3], vc0[3])
    HD = H * dh
    qkv = d["qkv"].view(len(seen), C, 3 * HD)
    for b in (0, 1, 2, 4):
        exp_k, exp_v = kc0[b].clone(), vc0[b].clone()
        for r in range(nvalid[b]):
            exp_k[(seen[b] + r) % hist], exp_v[(seen[b] + r) % hist] = qkv[b, r, HD:2 * HD], qkv[b, r, 2 * HD:]
        assert torch.equal(d["kc"][b], exp_k) and torch.equal(d["vc"][b], exp_v), b


@pytest.mark.parametrize("dtype", DT)
def test_chunk_attention_without_history_and_with_few_slots(dev, dtype):
    bar = dict(rtol=1e-4, atol=1e-5) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    out, ref, d = _attn_case(dev, dtype, 4, 8, 8, 4, 0, [0, 8, 12], [4, 3, 0], 3)  # hist = 0: the chunk sees itself only
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), **bar)
    K.stream_kv_append(d["qkv"], None, None, d["seen"], d["nv"], 3, 4, 4, 8, 0)
    # fewer slots than chunk rows (hist 2 < C 4): only the last two rows stay in the ring
    out, ref, d = _attn_case(dev, dtype, 2, 8, 8, 4, 2, [4, 0], [4, 4], 4)
    np.testing.assert_allclose(out.float().cpu().numpy(), ref.numpy(), **bar)
    K.stream_kv_append(d["qkv"], d["kc"], d["vc"], d["seen"], d["nv"], 2, 4, 2, 8, 2)
    torch.cuda.synchronize()
    qkv = d["qkv"].view(2, 4, 3 * 16)
    for b in range(2):
        for r in (2, 3):
            assert torch.equal(d["kc"][b, r % 2], qkv[b, r, 16:32]) and torch.equal(d["vc"][b, r % 2], qkv[b, r, 32:])


def test_attention_beyond_the_limits_is_an_error(dev):
    z = torch.zeros(8, device=dev)
    i = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(K._lib.TfasrUnsupported):
        K.stream_attn_fwd(z, z, z, z, z, z, i, i, 1, K.STREAM_MAX_CHUNK + 1, 1, 8, 4, 1.0)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("Kk", [7, 31])
def test_glu_dwconv_with_carried_state(dev, dtype, Kk):
    """state spanning several chunks (C = 4 < K - 1), streams idle in some steps, a partial chunk: the concatenated outputs equal the
    offline causal depthwise conv of each stream's valid rows.  Bar of test_glu_dwconv."""
    g = torch.Generator().manual_seed(Kk)
    B, C, d, steps = 3, 4, 144, 12
    w, bias = torch.randn(Kk, d, generator=g) * 0.2, torch.randn(d, generator=g) * 0.1
    plan = [[C, C if s % 2 == 0 else 0, (C if s < 7 else (3 if s == 7 else 0))] for s in range(steps)]
    state = torch.zeros(B, Kk - 1, d, dtype=dtype, device=dev)
    xs, ys = [[] for _ in range(B)], [[] for _ in range(B)]
    for s in range(steps):
        a = torch.randn(B * C, 2 * d, generator=g).to(dtype)
        before = state.clone()
        y = K.stream_glu_dwconv_fwd(a.to(dev), state, w.to(dev), bias.to(dev), _i32(plan[s], dev), B, C).view(B, C, d)
        for b in range(B):
            n = plan[s][b]
            xs[b].append(a.view(B, C, 2 * d)[b, :n].float())
            ys[b].append(y[b, :n].float().cpu())
            assert not y[b, n:].any()
            if n == 0:
                assert torch.equal(state[b], before[b])  # an idle stream's state: bit-equal
    for b in range(B):
        x = torch.cat(xs[b], 0)
        p, q = x.chunk(2, -1)
        gl = (p * torch.sigmoid(q)).to(dtype).float()
        ref = R.depthwise_conv1d_causal(gl[None], w, bias)[0]
        np.testing.assert_allclose(torch.cat(ys[b], 0).numpy(), ref.numpy(), **tol(dtype, (1e-4, 1e-5)))


def test_logmel_stream_with_and_without_the_carried_sample(dev):
    cfg = R.conformer_config("S")
    sig = np.stack(SO.noise(11, [0.5, 0.5, 0.5]))
    ref = R.log_mel(sig, cfg)  # [3, 50, 80]
    melw = R.mel_weight_matrix()
    consts = (torch.from_numpy(R.hann_periodic(400)).to(dev), torch.from_numpy(melw).to(dev), torch.from_numpy(R.mel_bands(melw)).to(dev), 160, 512, 0.97,
              1e-6, torch.float32)
    N, T0 = 160 * 9 + 400, 10
    # row 0 starts the utterance (no previous sample), row 1 continues at frame 7, row 2 holds the padded tail of the utterance
    starts = [0, 7 * 160, 40 * 160]
    buf = np.zeros((3, N), np.float32)
    nlen = []
    for b, s in enumerate(starts):
        seg = sig[b, s:s + N]
        buf[b, :len(seg)] = seg
        nlen.append(len(seg))
    prev = np.array([0.0, sig[1, starts[1] - 1], sig[2, starts[2] - 1]], np.float32)
    out = K.logmel_stream(torch.from_numpy(buf).to(dev), _i32(nlen, dev), torch.from_numpy(prev).to(dev), _i32([0, 1, 1], dev), T0, *consts)
    torch.cuda.synchronize()
    for b, s in enumerate(starts):
        np.testing.assert_allclose(out[b].cpu().numpy(), ref[b, s // 160:s // 160 + T0], atol=2e-5, rtol=0)
    # and the offline kernel is what it was: the same frames from the whole signal, bit for bit
    whole = K.logmel(torch.from_numpy(sig).to(dev), *consts)
    assert torch.equal(whole[0, :T0], out[0]) and torch.equal(whole[1, 7:7 + T0], out[1])
    # the periodic Hann window is zero at index 0, which hides the carried sample (column 0 is always a frame start); under a window that
    # is not, the carried sample is what makes a continued stream's first frame the offline frame
    rect = (torch.ones(400, device=dev),) + consts[1:]
    args = (torch.from_numpy(buf).to(dev), _i32(nlen, dev), torch.from_numpy(prev).to(dev))
    with_prev = K.logmel_stream(*args, _i32([0, 1, 1], dev), T0, *rect)
    without = K.logmel_stream(*args, _i32([0, 0, 0], dev), T0, *rect)
    whole = K.logmel(torch.from_numpy(sig).to(dev), *rect)
    assert torch.equal(with_prev[1], whole[1, 7:7 + T0]) and torch.equal(with_prev[0], whole[0, :T0])
    assert torch.equal(without[1, 1:], with_prev[1, 1:]) and not torch.equal(without[1, 0], with_prev[1, 0])


# =============================================================================================== models
def _tiny(dev, dtype, W=None, head="transducer", **over):
    cfg = configs.conformer_tiny(**{**SO.STREAM_OVER, **over}, head=head)
    cfg.time_masking, cfg.freq_masking = {}, {}
    model = (ConformerCTC if head == "ctc" else ConformerTransducer)(cfg, dev, dtype=dtype, seed=0)
    if W is not None:
        model.ps.import_keras(W)
    return model


def _feed(rec, sigs, piece):
    """all streams fed `piece` samples at a time (ragged ends), then finish -> (tokens per stream, encoder frames per stream)"""
    B = len(sigs)
    rec.encoded_log = []
    toks = [[] for _ in range(B)]
    frames_seen = []

    def take(out):
        for b in range(B):
            toks[b] += out.tokens[b, :int(out.tokens_length[b])].tolist()
        frames_seen.append(out.frames.tolist())

    n = max(len(s) for s in sigs)
    for p0 in range(0, n, piece):
        x = np.zeros((B, piece), np.float32)
        lens = []
        for b, s in enumerate(sigs):
            seg = s[p0:p0 + piece]
            x[b, :len(seg)] = seg
            lens.append(len(seg))
        take(rec.accept(torch.from_numpy(x), lens))
    take(rec.finish())
    enc = [torch.cat([e[b, :nv[b]] for e, nv in rec.encoded_log] + [rec.encoded_log[0][0][b, :0]], 0).float().cpu() for b in range(B)]
    return toks, enc, frames_seen[-1]


def _golden_utts(z):
    return [z["signals"][b, :int(z["signals_length"][b])] for b in range(z["signals"].shape[0])]


@pytest.mark.parametrize("dtype", DT)
def test_encoder_session_against_the_reference_made_golden(dev, dtype):
    """weights and signals[0] of the streaming wiring golden, 733 samples at a time, against eval/encoder[0] (the longest row of the
    reference's padded batch = that utterance alone); then all three utterances as three streams of one session against the f64 oracle
    of each alone.  Bars of tests/test_reference_wiring_gpu.py."""
    z, W64 = SO.load_golden()
    W32 = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("W/")}
    model = _tiny(dev, dtype, W32)
    prec = "f32" if dtype == torch.float32 else "bf16"
    bar = F32_BAR if dtype == torch.float32 else BF16_BAR
    utts = _golden_utts(z)
    _, enc, frames = _feed(model.stream(1, precision=prec), [utts[0]], 733)
    gold = z["eval/encoder"][0]
    assert enc[0].shape == gold.shape and frames == [gold.shape[0]]
    print(f"\n[stream] golden row 0, {prec}: rel L2 {_rel(enc[0].numpy(), gold):.3e} (bar {bar})")
    assert _rel(enc[0].numpy(), gold) < bar
    ocfg = SO.oracle_cfg(**SO.STREAM_OVER)
    _, enc, frames = _feed(model.stream(3, precision=prec), utts, 733)
    for b, sig in enumerate(utts):
        ref, _ = SO.offline_alone(sig, W64, ocfg)
        assert enc[b].shape == ref.shape and frames[b] == ref.shape[0]
        print(f"[stream] three streams, {prec}, utterance {b}: rel L2 vs oracle alone {_rel(enc[b].numpy(), ref.numpy()):.3e}")
        assert _rel(enc[b].numpy(), ref.numpy()) < bar


def _s_model(dev, dtype, **over):
    cfg = configs.conformer_s(chunk_size=16, history_size=64, num_blocks=4, dropout=0.0, **over)
    cfg.time_masking, cfg.freq_masking = {}, {}
    return ConformerTransducer(cfg, dev, dtype=dtype, seed=0)


S_SECONDS = [3.0, 10.0, 5.3, 7.7]


@pytest.mark.parametrize("dtype", DT)
def test_session_against_the_offline_path_at_s_dimensions(dev, dtype):
    """head 36, kernel 31, chunk 16, history 64, 4 blocks (batch norms on moving statistics), B = 4, ragged 3 to 10 s of seeded noise:
    the session's encoder frames against model.encode of each utterance alone."""
    model = _s_model(dev, dtype)
    prec = "f32" if dtype == torch.float32 else "bf16"
    bar = F32_BAR if dtype == torch.float32 else BF16_BAR
    sigs = SO.noise(3, S_SECONDS)
    _, enc, frames = _feed(model.stream(4, precision=prec), sigs, 16000)
    for b, sig in enumerate(sigs):
        ref, elen = model.encode(torch.from_numpy(sig)[None], torch.tensor([len(sig)]), precision=prec)
        ref = ref[0, :elen[0]].float().cpu()
        assert enc[b].shape == ref.shape and frames[b] == elen[0]
        r = _rel(enc[b].numpy(), ref.numpy())
        print(f"\n[stream] S dims {prec} utterance {b} ({S_SECONDS[b]} s): session vs model.encode alone rel L2 {r:.3e} (bar {bar})")
        assert r < bar


def test_arrival_does_not_matter_and_a_reused_slot_is_a_fresh_stream(dev):
    """the same audio 160, 733, 10 240 samples at a time and all at once: bit-equal encoder frames and tokens; a stream that takes the
    slot of a finished one after reset gives the frames it gives alone."""
    z, _ = SO.load_golden()
    W32 = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("W/")}
    model = _tiny(dev, torch.float32, W32)
    model.ps.p("joint/vocab/b")[0] += 0.5
    sigs = SO.noise(1, [1.7, 3.0, 2.2])
    base_t, base_e, _ = _feed(model.stream(3), sigs, 48000)
    assert sum(len(t) for t in base_t) > 0
    for piece in (160, 733, 10240):
        t, e, _ = _feed(model.stream(3), sigs, piece)
        assert t == base_t, piece
        for b in range(3):
            assert torch.equal(e[b], base_e[b]), (piece, b)
    # slot 1 finishes early, is reset, and takes utterance 0 while slot 0 is still running
    rec = model.stream(2)
    rec.encoded_log = []
    a, b_, c_ = sigs[1], sigs[2][:16000], sigs[0]
    rec.accept(torch.from_numpy(np.stack([a[:16000], b_])))
    rec.finish(rows=[1])
    with pytest.raises(RuntimeError, match="finished"):
        rec.accept(torch.from_numpy(np.zeros((2, 160), np.float32)), [0, 160])
    rec.reset(rows=[1])
    mark = len(rec.encoded_log)
    x = np.zeros((2, len(a) - 16000), np.float32)
    x[0] = a[16000:]
    x[1, :len(c_)] = c_
    rec.accept(torch.from_numpy(x), [len(a) - 16000, len(c_)])
    rec.finish()
    got0 = torch.cat([e[0, :nv[0]] for e, nv in rec.encoded_log], 0).cpu()
    got1 = torch.cat([e[1, :nv[1]] for e, nv in rec.encoded_log[mark:]], 0).cpu()
    assert got0.shape == base_e[1].shape and _rel(got0.numpy(), base_e[1].numpy()) < F32_BAR
    assert got1.shape == base_e[0].shape and _rel(got1.numpy(), base_e[0].numpy()) < F32_BAR


def test_latency_in_samples(dev):
    """encoder frame C (c + 1) - 1 needs 640 C (c + 1) + 240 samples; after finish frames = ceil(ceil(ceil(n / 160) / 2) / 2)."""
    model = _tiny(dev, torch.float32)
    C = model.cfg.chunk_size
    for c in (0, 1, 3):
        need = 640 * C * (c + 1) + 240
        rec = model.stream(1)
        out = rec.accept(torch.zeros(1, need - 1))
        assert out.frames.tolist() == [C * c]
        out = rec.accept(torch.ones(1, 1) * 0.1)
        assert out.frames.tolist() == [C * (c + 1)]
    for n in (1, 159, 160, 161, 640 * C + 239, 640 * C + 240, 5000, 12345):
        rec = model.stream(1)
        rec.accept(torch.zeros(1, n))
        out = rec.finish()
        assert out.frames.tolist() == [-(-(-(-(-(-n // 160)) // 2)) // 2)], n


# =============================================================================================== search
def _search_inputs(dev):
    z, _ = SO.load_golden()
    W32 = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("W/")}
    model = _tiny(dev, torch.float32, W32)
    model.ps.p("joint/vocab/b")[0] += 0.5  # the blank bias: an untrained model neither always speaks nor never
    sigs = SO.noise(1, [1.7, 3.0, 2.2, 2.6])
    encs = [model.encode(torch.from_numpy(s)[None], torch.tensor([len(s)])) for s in sigs]
    return model, sigs, [(e, int(l[0])) for e, l in encs]


def _tokens_of(out):
    t = out.tokens[0].tolist()
    return [v for v in t if v != 0]


def test_search_carry_single_stream_is_exact(dev):
    """B = 1: the offline f32 encoder output cut into chunks and searched chunk by chunk (mode 1, carried token and state) gives the
    tokens of recognize_encoded on the whole."""
    model, sigs, encs = _search_inputs(dev)
    mtpf = 3
    reached = False
    for (enc, n), sig in zip(encs, sigs):
        whole = _tokens_of(model.recognize_encoded(enc[:, :n], [n]))
        assert len(whole) >= len(sig) / 16000.0, "input condition: at least one token per second of audio"
        for C in (1, 2, 5):
            toks, tok, st = [], None, None
            for t in range(0, n, C):
                m = min(C, n - t)
                out = model.recognize_encoded(enc[:, t:t + m].contiguous(), [m], tok, st)
                new = _tokens_of(out)
                reached |= C == 1 and len(new) == mtpf
                toks += new
                tok, st = out.next_tokens, out.next_decoder_states
            assert toks == whole, C
    assert reached, "input condition: at least one frame reaches max_tokens_per_frame"


def test_search_mode_2_rows_equal_single_searches(dev):
    """B = 4, mode 2, ragged nframes with one row at 0 in every step: row b equals recognize_encoded(enc[b:b+1], elen[b:b+1])."""
    model, sigs, encs = _search_inputs(dev)
    B, C = 4, 5
    rec = model.stream(B)
    whole = [_tokens_of(model.recognize_encoded(e[:, :n], [n])) for e, n in encs]
    assert all(len(w) >= len(s) / 16000.0 for w, s in zip(whole, sigs))
    pos, toks, step = [0] * B, [[] for _ in range(B)], 0
    d = encs[0][0].shape[2]
    while any(pos[b] < encs[b][1] for b in range(B)):
        chunk = torch.zeros(B, C, d, device=dev)
        nv = []
        for b in range(B):
            n = 0 if b == step % B else min(C - (b % 2), encs[b][1] - pos[b])  # one row idle per step, rows of different length
            chunk[b, :n] = encs[b][0][0, pos[b]:pos[b] + n]
            pos[b] += n
            nv.append(n)
        step += 1
        if max(nv) == 0:
            continue
        new = rec._search(chunk, _i32(nv, dev), nv)
        for b in range(B):
            toks[b] += new[b]
    assert toks == whole


# =============================================================================================== end to end
def _assert_margin(W64, ocfg, sigs):
    """near-ties are excluded by construction, not by a looser comparison: the smallest best - second-best log-probability over all
    decisions of the f64 oracle run must be far above the f32 path's error"""
    refs = [SO.oracle_decode(s, W64, ocfg) for s in sigs]
    gap = min(g for _, _, g in refs)
    print(f"\n[stream] smallest decision margin of the f64 oracle: {gap:.3e}")
    assert gap > 1e-3, "input condition: pick another seed"
    return [t for _, t, _ in refs]


def test_end_to_end_tokens_equal_offline_recognize_tiny(dev):
    z, W64 = SO.load_golden()
    W32 = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("W/")}
    W64["joint/vocab/b"][0] += 0.5
    sigs = _golden_utts(z) + SO.noise(1, [1.7, 3.0, 2.2])
    oracle_toks = _assert_margin(W64, SO.oracle_cfg(**SO.STREAM_OVER), sigs)
    for dtype in DT:
        model = _tiny(dev, dtype, W32)
        model.ps.p("joint/vocab/b")[0] += 0.5
        prec = "f32" if dtype == torch.float32 else "bf16"
        toks, _, _ = _feed(model.stream(len(sigs), precision=prec), sigs, 4000)
        alone = [_tokens_of(model.recognize(PredictInput(torch.from_numpy(s)[None], torch.tensor([len(s)])), precision=prec)) for s in sigs]
        same = sum(a == b for a, b in zip(toks, alone))
        print(f"[stream] tiny {prec}: {same} of {len(sigs)} utterances with tokens equal to recognize alone")
        if dtype == torch.float32:
            assert toks == alone and toks == oracle_toks


S_LOGIT_SCALE, S_BLANK_SHIFT = 30.0, 21.0  # a random-init vocabulary layer has near-tied classes: spread them (input condition below)


def test_end_to_end_tokens_equal_offline_recognize_s_dimensions(dev):
    sigs = SO.noise(3, S_SECONDS)
    for dtype in DT:
        model = _s_model(dev, dtype)
        model.ps.p("joint/vocab/w").mul_(S_LOGIT_SCALE)
        model.ps.p("joint/vocab/b")[0] += S_BLANK_SHIFT
        prec = "f32" if dtype == torch.float32 else "bf16"
        if dtype == torch.float32:
            W64 = {k: v.double().cpu() for k, v in model.ps.export_keras().items()}
            oracle_toks = _assert_margin(W64, SO.cfg_to_oracle(model.cfg), sigs)
            assert all(len(t) >= s for t, s in zip(oracle_toks, S_SECONDS))
        toks, _, _ = _feed(model.stream(4, precision=prec), sigs, 10240)
        alone = [_tokens_of(model.recognize(PredictInput(torch.from_numpy(s)[None], torch.tensor([len(s)])), precision=prec)) for s in sigs]
        same = sum(a == b for a, b in zip(toks, alone))
        print(f"[stream] S dims {prec}: {same} of {len(sigs)} utterances with tokens equal to recognize alone")
        if dtype == torch.float32:
            assert toks == alone and toks == oracle_toks


# =============================================================================================== CTC
def test_ctc_merge_across_the_chunk_boundary(dev):
    """the same non-blank class straddling a boundary merges; a blank on the boundary between two equal classes keeps both."""
    V = 6
    seqs = [[2, 2, 2, 2, 3, 0, 3, 3], [1, 1, 1, 0, 1, 1, 4, 4], [0, 5, 5, 5, 5, 5, 5, 0]]  # chunks of 4: [..2|2..] merges, [..0|1..] after 1 does not
    logits = torch.full((3, 8, V), -5.0)
    for b, s in enumerate(seqs):
        for t, c in enumerate(s):
            logits[b, t, c] = 5.0
    logits = logits.to(dev)
    whole, wlen = K.ctc_greedy_decode(logits, _i32([8, 8, 8], dev), blank=0)
    expect = [[2, 3, 3], [1, 1, 4], [5]]
    assert [whole[b, :int(wlen[b])].tolist() for b in range(3)] == expect
    last = torch.full((3,), -1, dtype=torch.int32, device=dev)
    got = [[] for _ in range(3)]
    for t0, lens in ((0, [4, 4, 4]), (4, [0, 4, 4]), (4, [4, 0, 0])):  # (rows idle in a step keep their class)
        before = last.clone()
        toks, tl = K.ctc_greedy_decode_carry(logits[:, t0:t0 + 4].contiguous(), _i32(lens, dev), last, blank=0)
        for b in range(3):
            got[b] += toks[b, :int(tl[b])].tolist()
            if lens[b] == 0:
                assert int(last[b]) == int(before[b])
    assert got == expect


def test_ctc_session_equals_recognize_alone(dev):
    model = _tiny(dev, torch.float32, head="ctc")
    sigs = SO.noise(5, [1.7, 3.0, 2.2])
    toks, _, _ = _feed(model.stream(3), sigs, 4000)
    for b, s in enumerate(sigs):
        out = model.recognize(PredictInput(torch.from_numpy(s)[None], torch.tensor([len(s)])))
        assert toks[b] == _tokens_of(out), b
    assert sum(len(t) for t in toks) > 0


# =============================================================================================== refusals
def test_refusals_at_session_creation(dev):
    with pytest.raises(ValueError, match="chunk_size is None"):
        _tiny(dev, torch.float32, chunk_size=None, history_size=None).stream()
    with pytest.raises(ValueError, match="unlimited history"):
        _tiny(dev, torch.float32, history_size=-1).stream()
    with pytest.raises(ValueError, match="limits"):
        _tiny(dev, torch.float32, chunk_size=K.STREAM_MAX_CHUNK + 1).stream()
    with pytest.raises(ValueError, match="limits"):
        _tiny(dev, torch.float32, chunk_size=16, history_size=K.STREAM_MAX_KEYS).stream_state(2)
    with pytest.raises(NotImplementedError, match="squeeze-and-excite"):
        ContextNetTransducer(configs.contextnet_tiny(), dev, dtype=torch.float32, seed=0).stream()
    rec = _tiny(dev, torch.float32).stream(1)
    rec.accept(torch.zeros(1, 4000))
    rec.finish()
    with pytest.raises(RuntimeError, match="finished"):
        rec.accept(torch.zeros(1, 160))
    rec.reset()
    assert rec.accept(torch.zeros(1, 4000)).frames.tolist() == [4]


def test_encoder_state_travels_through_the_predict_schemas(dev):
    model = _tiny(dev, torch.float32)
    rec = model.stream(1)
    rec.accept(torch.from_numpy(SO.noise(2, [0.5])[0])[None])
    st = rec.encoder_state()
    sig = torch.from_numpy(SO.noise(2, [0.3])[0])[None]
    out = model.recognize(PredictInput(sig, torch.tensor([sig.shape[1]]), previous_encoder_states=st))
    assert out.next_encoder_states is st
    assert model.recognize(PredictInput(sig, torch.tensor([sig.shape[1]]))).next_encoder_states is None
    rec2 = model.stream(1)
    rec2.set_encoder_state(out.next_encoder_states)
    for a, b in zip(rec2.encoder_state(), st):
        assert torch.equal(a, b)


# =============================================================================================== the encoder-stream interface
class _InterfaceOnly:
    """an encoder state that shows the session the members of streaming.EncoderStream's interface and nothing else"""
    MEMBERS = ("check", "step_rule", "f32_features", "prepare", "encode", "uses_final", "reset", "export", "load")

    def __init__(self, state):
        self._state = state

    def __getattr__(self, name):
        if name not in self.MEMBERS:
            raise AttributeError(f"the session asked its encoder state for {name!r}, which is not in the interface")
        return getattr(self._state, name)


def test_the_session_reads_its_encoder_through_the_interface_alone(dev):
    """a Jasper session whose state is wrapped so that only the interface's members exist gives what a plain session gives: every
    StreamOutput, the encoder frames and the encoder state, under ragged lengths and pieces of 1 and 4001 samples"""
    from test_jasper_gpu import build

    model = build(dev, torch.bfloat16)
    model.decode_precision = "bf16"
    rng = np.random.default_rng(5)
    sigs = [np.clip(rng.standard_normal(n) * 0.1, -1, 1).astype(np.float32) for n in (8000, 6001)]  # 0.5 s, and a ragged end
    for piece in (1, 4001):
        recs = [model.stream(2, chunk_frames=8, precision="bf16") for _ in range(2)]
        recs[0].state = _InterfaceOnly(recs[0].state)
        with pytest.raises(AttributeError, match="not in the interface"):
            recs[0].state.tails
        outs = []
        for rec in recs:
            rec.encoded_log = []
            got, pos = [], [0, 0]
            while any(pos[b] < len(sigs[b]) for b in range(2)):
                x, lens = np.zeros((2, piece), np.float32), []
                for b in range(2):
                    seg = sigs[b][pos[b]:pos[b] + piece]
                    x[b, :len(seg)] = seg
                    lens.append(len(seg))
                    pos[b] += len(seg)
                got.append(rec.accept(torch.from_numpy(x), lens))
            got.append(rec.finish())
            outs.append(got)
        assert len(outs[0]) == len(outs[1]) and recs[0].chunks_run == recs[1].chunks_run > 4
        for a, b in zip(*outs):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert outs[0][-1].frames.tolist() == [25, 19]  # ceil(50 / 2) and ceil(38 / 2) encoder frames
        for (ea, na), (eb, nb) in zip(recs[0].encoded_log, recs[1].encoded_log):
            assert na == nb and torch.equal(ea, eb)
        sa, sb = recs[0].encoder_state(), recs[1].encoder_state()
        assert len(sa) == len(sb) > 0 and all(torch.equal(x, y) for x, y in zip(sa, sb))
