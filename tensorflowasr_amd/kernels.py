"""Thin torch-tensor -> C-ABI adapters (raw device pointers + the current HIP stream).

Every function here requires CUDA(HIP) tensors and fails loudly otherwise: there is no CPU fallback.
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import ACT_FACTOR, ACT_NONE, ACT_SIGMOID, ACT_SWISH, ACT_TANH, ACT_TANH_OUT, TFASR_BF16, TFASR_F32, GemmArgs, check  # noqa: F401

_WS_CACHE = {}
_SPLITK_WS = False  # k-slices of a split product through a workspace (deterministic sums; measured slower than the f32 atomics: tests set it)


def _dt(t):
    if t.dtype == torch.float32:
        return TFASR_F32
    if t.dtype == torch.bfloat16:
        return TFASR_BF16
    raise TypeError(f"unsupported activation dtype {t.dtype}")


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.TfasrError("tensorflowasr_amd ops need HIP device tensors (no CPU fallback on the product path)")
    if not t.is_contiguous():
        raise _lib.TfasrError(f"non-contiguous tensor passed to a HIP kernel (shape {tuple(t.shape)}, strides {t.stride()})")
    return ctypes.c_void_p(t.data_ptr())


def _pv(t):
    """pointer of a strided VIEW (the kernel receives the strides explicitly)"""
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.TfasrError("tensorflowasr_amd ops need HIP device tensors (no CPU fallback on the product path)")
    return ctypes.c_void_p(t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The HIP stream torch currently launches on (raw hipStream_t).  torch.cuda.current_stream() builds a Stream object per
    call (~9 us); the raw query is one C call, which matters at ~1500 launches per train step."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device, tag="ws"):
    """Grow-only per-(device, tag) scratch buffer (uint8)."""
    key = (str(device), tag)
    buf = _WS_CACHE.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _WS_CACHE[key] = buf
    return buf


# --------------------------------------------------------------------------------------------- RNN-T
def rnnt_loss_workspace_size(B, T, U1, V):
    n = ctypes.c_size_t(0)
    check(_lib.load().tfasr_rnnt_loss_workspace_size(B, T, U1, V, ctypes.byref(n)), "rnnt_loss_workspace_size")
    return n.value


def rnnt_loss_fwd_bwd(logits, labels, label_len, logit_len, grad_scale=None, grads=None, want_grads=True, blank=0):
    """logits [B,T,U1,V] (f32|bf16, contiguous) -> (costs [B] f32, grads or None). grads may be `logits` (in place)."""
    assert logits.dim() == 4 and logits.is_contiguous()
    B, T, U1, V = logits.shape
    assert labels.shape == (B, U1 - 1) and labels.dtype == torch.int32 and labels.is_contiguous()
    assert label_len.dtype == torch.int32 and logit_len.dtype == torch.int32
    costs = torch.empty(B, dtype=torch.float32, device=logits.device)
    if want_grads and grads is None:
        grads = torch.empty_like(logits)
    nbytes = rnnt_loss_workspace_size(B, T, U1, V)
    ws = workspace(nbytes, logits.device, "rnnt")
    check(
        _lib.load().tfasr_rnnt_loss(
            _p(logits), _p(grads) if want_grads else None, _p(labels), _p(label_len), _p(logit_len),
            _p(grad_scale), B, T, U1, V, blank, _dt(logits), _p(costs), _p(ws), ws.numel(), _stream()),
        "rnnt_loss")
    return costs, (grads if want_grads else None)


def rnnt_row_labels(labels, label_len, logit_len, cell_off, total_cells, T, V):
    """[total_cells] i32: the label id each packed lattice row can emit (-1: none)."""
    B, U = labels.shape
    out = torch.empty(total_cells, dtype=torch.int32, device=labels.device)
    check(_L().tfasr_rnnt_row_labels(_p(labels), _p(label_len), _p(logit_len), _p(cell_off), total_cells, B, T, U + 1, V, _p(out), _stream()),
          "rnnt_row_labels")
    return out


def rnnt_loss_packed(logits, labels, label_len, logit_len, cell_off, total_cells, T, grad_scale=None, grads=None, want_grads=True, blank=0,
                     stats=None):
    """logits [total_cells, V] over the packed lattice (see include/tfasr_hip.h) -> (costs [B], grads).  stats = (lse_part, pick)
    from the projection GEMM's epilogue (kernels.gemm lse=...): skips the first pass over the logits."""
    assert logits.dim() == 2 and logits.is_contiguous() and cell_off.dtype == torch.int64
    B, U = labels.shape
    V = logits.shape[1]
    costs = torch.empty(B, dtype=torch.float32, device=logits.device)
    if want_grads and grads is None:
        grads = torch.empty_like(logits)
    nbytes = rnnt_loss_workspace_size(1, total_cells, 1, V)
    ws = workspace(nbytes, logits.device, "rnnt")
    if stats is not None:
        part, pick = stats
        check(_lib.load().tfasr_rnnt_loss_packed_stats(
            _p(logits), _p(grads) if want_grads else None, _p(labels), _p(label_len), _p(logit_len), _p(grad_scale), _p(cell_off),
            total_cells, _p(part), part.shape[1], _p(pick), B, T, U + 1, V, blank, _dt(logits), _p(costs), _p(ws), ws.numel(), _stream()),
            "rnnt_loss_packed_stats")
        return costs, (grads if want_grads else None)
    check(_lib.load().tfasr_rnnt_loss_packed(
        _p(logits), _p(grads) if want_grads else None, _p(labels), _p(label_len), _p(logit_len), _p(grad_scale), _p(cell_off),
        total_cells, B, T, U + 1, V, blank, _dt(logits), _p(costs), _p(ws), ws.numel(), _stream()), "rnnt_loss_packed")
    return costs, (grads if want_grads else None)


def rnnt_loss_packed_coef(labels, label_len, logit_len, cell_off, total_cells, T, V, stats, grad_scale=None, blank=0):
    """The loss WITHOUT logits (joint "recompute" variant): costs [B] and the per-row coefficients [total_cells, 4] f32 from which a
    re-computed logit tile becomes the gradient (gemm(..., rgrad=(coef, row_label)))."""
    B, U = labels.shape
    part, pick = stats
    costs = torch.empty(B, dtype=torch.float32, device=part.device)
    coef = torch.empty(total_cells, 4, dtype=torch.float32, device=part.device)
    ws = workspace(rnnt_loss_workspace_size(1, total_cells, 1, V), part.device, "rnnt")
    check(_lib.load().tfasr_rnnt_loss_packed_coef(_p(labels), _p(label_len), _p(logit_len), _p(grad_scale), _p(cell_off), total_cells, _p(part),
                                                  part.shape[1], _p(pick), B, T, U + 1, V, blank, _p(costs), _p(coef), _p(ws), ws.numel(), _stream()),
          "rnnt_loss_packed_coef")
    return costs, coef


# ------------------------------------------------------------------------------------ forced alignment
def rnnt_align_workspace_size(B, T, U1, V):
    n = ctypes.c_size_t(0)
    check(_lib.load().tfasr_rnnt_align_workspace_size(B, T, U1, V, ctypes.byref(n)), "rnnt_align_workspace_size")
    return n.value


def ctc_align_workspace_size(B, T, U, V):
    n = ctypes.c_size_t(0)
    check(_lib.load().tfasr_ctc_align_workspace_size(B, T, U, V, ctypes.byref(n)), "ctc_align_workspace_size")
    return n.value


def _align_check(st, what):
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"{what}: shape outside what the alignment kernels hold (see include/tfasr_hip.h)")
    check(st, what)


def _rnnt_align_io(labels_shape, label_len, logit_len, cell_off, dev):
    B, U = labels_shape
    assert label_len.dtype == torch.int32 and logit_len.dtype == torch.int32 and label_len.shape == (B,) and logit_len.shape == (B,)
    assert cell_off is None or (cell_off.dtype == torch.int64 and cell_off.numel() >= B)
    frames = torch.empty(B, U, dtype=torch.int32, device=dev)
    label_lp = torch.empty(B, U, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    return frames, label_lp, score


def rnnt_align_lattice(blank_lp, truth_lp, label_len, logit_len, T=None, U1=None, cell_off=None):
    """Viterbi walk over caller-supplied lattice log-probabilities (f32): dense [B,T,U1], or packed [total_cells] with cell_off [B(+1)]
    int64 and the padded T / U1 given.  -> (frames [B,U1-1] i32, label_lp [B,U1-1] f32, score [B] f32); on a tie a label is emitted as late as possible."""
    assert blank_lp.dtype == torch.float32 and truth_lp.dtype == torch.float32 and blank_lp.shape == truth_lp.shape
    if cell_off is None:
        assert blank_lp.dim() == 3
        B, T, U1 = blank_lp.shape
        total = B * T * U1
    else:
        assert blank_lp.dim() == 1 and T is not None and U1 is not None
        B, total = label_len.shape[0], blank_lp.shape[0]
    frames, label_lp, score = _rnnt_align_io((B, U1 - 1), label_len, logit_len, cell_off, blank_lp.device)
    ws = workspace(rnnt_align_workspace_size(B, T, U1, 2), blank_lp.device, "align")
    _align_check(_lib.load().tfasr_rnnt_align_lattice(_p(blank_lp), _p(truth_lp), _p(label_len), _p(logit_len), _p(cell_off), total, B, T, U1,
                                                      _p(frames), _p(label_lp), _p(score), _p(ws), ws.numel(), _stream()), "rnnt_align_lattice")
    return frames, label_lp, score


def rnnt_align(logits, labels, label_len, logit_len, T=None, cell_off=None, blank=0):
    """Forced alignment from logits (f32 | bf16): dense [B,T,U1,V], or packed [total_cells,V] with cell_off and the padded T.
    labels [B,U1-1] i32.  -> (frames, label_lp, score) as rnnt_align_lattice."""
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.dim() == 2
    B, U = labels.shape
    if cell_off is None:
        assert logits.dim() == 4 and logits.shape[0] == B and logits.shape[2] == U + 1
        T, V = logits.shape[1], logits.shape[3]
        total = B * T * (U + 1)
    else:
        assert logits.dim() == 2 and T is not None
        total, V = logits.shape
    frames, label_lp, score = _rnnt_align_io((B, U), label_len, logit_len, cell_off, logits.device)
    ws = workspace(rnnt_align_workspace_size(B, T, U + 1, V), logits.device, "align")
    _align_check(_lib.load().tfasr_rnnt_align(_p(logits), _p(labels), _p(label_len), _p(logit_len), _p(cell_off), total, B, T, U + 1, V, blank,
                                              _dt(logits), _p(frames), _p(label_lp), _p(score), _p(ws), ws.numel(), _stream()), "rnnt_align")
    return frames, label_lp, score


def rnnt_align_stats(stats, labels, label_len, logit_len, T, V, cell_off=None, blank=0):
    """Forced alignment from the vocabulary GEMM's statistics epilogue (stats = (lse_part [rows,parts,2], pick [rows,2]) of
    gemm(..., out=None, lse=...)): the logits never exist.  Rows are the lattice nodes, dense or packed (cell_off)."""
    part, pick = stats
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.dim() == 2
    B, U = labels.shape
    total = part.shape[0]
    assert cell_off is not None or total == B * T * (U + 1)
    frames, label_lp, score = _rnnt_align_io((B, U), label_len, logit_len, cell_off, part.device)
    ws = workspace(rnnt_align_workspace_size(B, T, U + 1, V), part.device, "align")
    _align_check(_lib.load().tfasr_rnnt_align_stats(_p(part), part.shape[1], _p(pick), _p(labels), _p(label_len), _p(logit_len), _p(cell_off), total,
                                                    B, T, U + 1, V, blank, _p(frames), _p(label_lp), _p(score), _p(ws), ws.numel(), _stream()),
                 "rnnt_align_stats")
    return frames, label_lp, score


def ctc_align(logits, labels, label_len, logit_len, blank=0, normalized=False):
    """CTC forced alignment of logits [B,T,V] (f32 | bf16; normalized=True: log-probabilities already) to labels [B,U] i32.
    -> (start [B,U] i32, end [B,U] i32, label_lp [B,U] f32, score [B] f32); ties take the smallest move, the final blank at the end."""
    assert logits.dim() == 3 and labels.dim() == 2 and labels.dtype == torch.int32 and labels.is_contiguous()
    B, T, V = logits.shape
    U = labels.shape[1]
    assert labels.shape[0] == B and label_len.dtype == torch.int32 and logit_len.dtype == torch.int32
    dev = logits.device
    start = torch.empty(B, U, dtype=torch.int32, device=dev)
    end = torch.empty(B, U, dtype=torch.int32, device=dev)
    label_lp = torch.empty(B, U, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    ws = workspace(ctc_align_workspace_size(B, T, U, V), dev, "align")
    _align_check(_lib.load().tfasr_ctc_align(_p(logits), _p(labels) if U else None, _p(label_len), _p(logit_len), B, T, U, V, blank, _dt(logits),
                                             1 if normalized else 0, _p(start) if U else None, _p(end) if U else None, _p(label_lp) if U else None,
                                             _p(score), _p(ws), ws.numel(), _stream()), "ctc_align")
    return start, end, label_lp, score


ALIGN_CTC_MAX_U = 511  # TFASR_ALIGN_CTC_MAX_U


def row_lse_entropy(x):
    """Log-sum-exp and entropy in nats of every row of x [..., V] (f32 | bf16, f32 arithmetic) -> (lse [...], entropy [...]) f32: a frame's
    definitions in ctc_greedy_decode_detail, the lse bit for bit the one ctc_align subtracts (tfasr_row_lse_entropy)."""
    assert x.dim() >= 1 and x.is_contiguous()
    V = x.shape[-1]
    rows = x.numel() // V
    lse = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    ent = torch.empty_like(lse)
    check(_lib.load().tfasr_row_lse_entropy(_p(x), rows, V, _dt(x), _p(lse), _p(ent), _stream()), "row_lse_entropy")
    return lse, ent


def ctc_nbest_align_workspace_size(B, P, T, U, V):
    n = ctypes.c_size_t(0)
    _align_check(_lib.load().tfasr_ctc_nbest_align_workspace_size(B, P, T, U, V, ctypes.byref(n)), "ctc_nbest_align_workspace_size")
    return n.value


def ctc_nbest_align(logits, logit_len, tokens, lengths, blank=0, max_labels=None):
    """CTC forced alignment of an n-best list to ONE copy of its utterance's logits (tfasr_ctc_nbest_align): logits [B,T,V] (f32 | bf16),
    logit_len [B] i32, tokens [B,P,W] i32 (a search's token array, read in place through its row stride), lengths [B,P] i32.  Columns past
    TFASR_ALIGN_CTC_MAX_U are not aligned.  -> (start, end [B,P,W] i32, label_lp, label_entropy [B,P,W] f32, score [B,P] f32): per
    path what ctc_align gives for (logits[b], tokens[b,p], logit_len[b]), bit for bit, plus the mean frame entropy of every label's span.
    lengths < 0 (a dead path) or > min(W, TFASR_ALIGN_CTC_MAX_U): score -inf, spans -1, zeros.  max_labels = U <= W: only the first U
    columns are label columns (longer paths are dead) and the outputs are [B,P,U]; U > TFASR_ALIGN_CTC_MAX_U raises TfasrUnsupported.
    max_labels is public on purpose: it is the C entry point's U beside ldl = W, for a caller who knows a bound on the hypotheses'
    lengths (the walk runs one thread per state of the label width) or wants the C call's own refusal of a width."""
    assert logits.dim() == 3 and tokens.dim() == 3 and tokens.dtype == torch.int32 and tokens.is_contiguous()
    B, T, V = logits.shape
    P, W = tokens.shape[1], tokens.shape[2]
    assert tokens.shape[0] == B and lengths.shape == (B, P) and lengths.dtype == torch.int32 and logit_len.dtype == torch.int32
    assert lengths.is_contiguous() and logit_len.shape == (B,)
    dev = logits.device
    U = min(W, ALIGN_CTC_MAX_U) if max_labels is None else int(max_labels)
    assert 0 <= U <= W
    start = torch.empty(B, P, U, dtype=torch.int32, device=dev)
    end = torch.empty(B, P, U, dtype=torch.int32, device=dev)
    label_lp = torch.empty(B, P, U, dtype=torch.float32, device=dev)
    label_ent = torch.empty(B, P, U, dtype=torch.float32, device=dev)
    score = torch.empty(B, P, dtype=torch.float32, device=dev)
    ws = workspace(ctc_nbest_align_workspace_size(B, P, T, U, V), dev, "align")
    q = (lambda t: _p(t) if U else None)
    _align_check(_lib.load().tfasr_ctc_nbest_align(_p(logits), _p(logit_len), q(tokens), W, _p(lengths), B, P, T, U, V, blank, _dt(logits), q(start),
                                                   q(end), q(label_lp), q(label_ent), _p(score), _p(ws), ws.numel(), _stream()), "ctc_nbest_align")
    if max_labels is None and U < W:  # the columns no walk reaches: no label sits there
        def wide(t, fill):
            full = torch.full((B, P, W), fill, dtype=t.dtype, device=dev)
            full[:, :, :U] = t
            return full
        start, end, label_lp, label_ent = wide(start, -1), wide(end, -1), wide(label_lp, 0.0), wide(label_ent, 0.0)
    return start, end, label_lp, label_ent, score


# ------------------------------------------------------------------------------------------ scoring
def _edit_check(st, what):
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"{what}: a sequence width above TFASR_EDIT_MAX_LEN (see include/tfasr_hip.h)")
    check(st, what)


def edit_distance_workspace_size(P, N, M):
    n = ctypes.c_size_t(0)
    _edit_check(_lib.load().tfasr_edit_distance_workspace_size(P, N, M, ctypes.byref(n)), "edit_distance_workspace_size")
    return n.value


def edit_distance(hyp, ref, hyp_len=None, ref_len=None, skip_id=-1):
    """Edit distance of hyp [P,N] against ref [P,M] (i32, device) -> counts [P,5] i32: distance, hits, substitutions, deletions,
    insertions (of the minimum-distance alignment with the most hits).  A side without lengths is compacted on the device: entries
    < 0 and entries == skip_id are dropped.  Widths above TFASR_EDIT_MAX_LEN raise TfasrUnsupported."""
    for t in (hyp, ref, hyp_len, ref_len):
        if t is not None and not t.is_cuda:
            raise _lib.TfasrError("tensorflowasr_amd ops need HIP device tensors (no CPU fallback on the product path)")
    assert hyp.dim() == 2 and ref.dim() == 2 and hyp.shape[0] == ref.shape[0] and hyp.dtype == torch.int32 and ref.dtype == torch.int32
    P, N, M = hyp.shape[0], hyp.shape[1], ref.shape[1]
    for ln in (hyp_len, ref_len):
        assert ln is None or (ln.dtype == torch.int32 and ln.shape == (P,))
    counts = torch.empty(P, 5, dtype=torch.int32, device=hyp.device)
    if P == 0:
        return counts
    ws = workspace(edit_distance_workspace_size(P, N, M), hyp.device, "edit")
    # an empty tensor has no storage: a width of 0 is never read, the pointer only has to be non-null
    _edit_check(_lib.load().tfasr_edit_distance(_p(hyp) if N else _p(counts), _p(hyp_len), _p(ref) if M else _p(counts), _p(ref_len), P, N, M,
                                                 int(skip_id), _p(counts), _p(ws), ws.numel(), _stream()), "edit_distance")
    return counts


# ---------------------------------------------------------------------------------------------- GEMM
def gemm(A, B, out, M, N, K, lda, ldb, ldd, trans_a=False, trans_b=False, bias=None, res=None, dact_z=None,
         prez=None, alpha=1.0, beta=1.0, act=ACT_NONE, dact=ACT_NONE, nb1=1, nb2=1, sA=(0, 0), sB=(0, 0), sD=(0, 0),
         accumulate=False, split_k=1, drop_p=0.0, drop_seed=0, colsum=None, lse=None, seg=None, rgrad=None, bns=None, row_tiles=None,
         k_tiles=None):
    """Raw strided (two-level batched) GEMM; see include/tfasr_hip.h.  bns = (x [M, N], fin [4N] f32, out [copies, 2N] f32): the BatchNorm
    backward sums of the output in the epilogue (tfasr_gemm_args.bns_*; raises TfasrUnsupported when the product is not the plain NT one).  lse = (lse_part [M, parts, 2] f32, row_label [M] i32,
    pick [M, 2] f32): fused log-softmax statistics of the output rows (raises TfasrUnsupported when the fast path cannot); with it
    `out` may be None (statistics only).  rgrad = (coef [M, 4] f32, row_label [M] i32): the product is a re-computed logit tile and the
    epilogue stores the RNN-T loss gradient instead (tfasr_gemm_args.rgrad_coef).  k_tiles: i32 device tensor, the ascending 256-row blocks
    of K a transposed-A weight gradient sums over (tfasr_gemm_args.k_tiles; raises TfasrUnsupported for any other product)."""
    a = _gemm_args(A, B, out, M, N, K, lda, ldb, ldd, trans_a, trans_b, bias, res, dact_z, prez, alpha, beta, act, dact, nb1, nb2, sA, sB, sD,
                   accumulate, split_k, drop_p, drop_seed, colsum, k_tiles, lse, seg, rgrad, bns, row_tiles)
    st = _lib.load().tfasr_gemm(ctypes.byref(a), _stream())
    if (lse is not None or seg is not None or rgrad is not None or bns is not None or k_tiles is not None) and st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported("gemm: fused row statistics / K-segments / gradient epilogue / K-block table are not available for this product")
    check(st, "gemm")
    return out


def gemm_route(ncu=0, **kw):
    """The kernel tfasr_gemm takes for gemm(**kw) on a part with `ncu` compute units (0: the current device), as the library itself says
    (tfasr_gemm_route; the rules: csrc/gemm_route.h): a _lib.GemmRouteInfo - status, family, layout, tile width, epilogue bits, grid, LDS,
    launch count.  Nothing is launched."""
    info = _lib.GemmRouteInfo()
    _lib.load().tfasr_gemm_route(ctypes.byref(_gemm_args(**kw)), int(ncu), ctypes.byref(info))
    return info


def gemm_group_route(calls, ncu=0):
    """(status, launches) of gemm_group(calls) (tfasr_gemm_group_route); nothing is launched"""
    arr = (GemmArgs * len(calls))()
    for i, kw in enumerate(calls):
        arr[i] = _gemm_args(**kw)
    n = ctypes.c_int(0)
    st = _lib.load().tfasr_gemm_group_route(arr, len(calls), int(ncu), ctypes.byref(n))
    return st, n.value


def gemm_group(calls):
    """Several independent products in one launch when they qualify (tfasr_gemm_group: bf16 weight gradients), else one by
    one.  `calls` = list of dicts with gemm()'s keyword arguments.  With k_tiles in the calls a product the library cannot run over the
    table raises TfasrUnsupported (nothing of that product has been launched; earlier products of the list may have been)."""
    arr = (GemmArgs * len(calls))()
    for i, kw in enumerate(calls):
        arr[i] = _gemm_args(**kw)
    st = _lib.load().tfasr_gemm_group(arr, len(calls), _stream())
    if st == _lib.STATUS_UNSUPPORTED and any(kw.get("k_tiles") is not None for kw in calls):
        raise _lib.TfasrUnsupported("gemm_group: K-block table not available for these products")
    check(st, "gemm_group")


def _gemm_args(A, B, out, M, N, K, lda, ldb, ldd, trans_a=False, trans_b=False, bias=None, res=None, dact_z=None,
               prez=None, alpha=1.0, beta=1.0, act=ACT_NONE, dact=ACT_NONE, nb1=1, nb2=1, sA=(0, 0), sB=(0, 0), sD=(0, 0),
               accumulate=False, split_k=1, drop_p=0.0, drop_seed=0, colsum=None, k_tiles=None, lse=None, seg=None, rgrad=None, bns=None,
               row_tiles=None):
    a = GemmArgs()
    a.A, a.B, a.D = A.data_ptr(), B.data_ptr(), (out.data_ptr() if out is not None else None)
    a.bias = bias.data_ptr() if bias is not None else None
    a.res = res.data_ptr() if res is not None else None
    a.dact_z = dact_z.data_ptr() if dact_z is not None else None
    a.prez = prez.data_ptr() if prez is not None else None
    a.M, a.N, a.K = M, N, K
    a.lda, a.ldb, a.ldd = lda, ldb, ldd
    a.trans_a, a.trans_b = int(trans_a), int(trans_b)
    a.nb1, a.nb2 = nb1, nb2
    a.sA1, a.sA2, a.sB1, a.sB2, a.sD1, a.sD2 = sA[0], sA[1], sB[0], sB[1], sD[0], sD[1]
    a.alpha, a.beta = alpha, beta
    a.act, a.dact = act, dact
    a.dtype = _dt(A)
    assert B.dtype == A.dtype and A.is_cuda and B.is_cuda and (out is None or out.is_cuda)
    a.out_f32 = int(out is not None and out.dtype == torch.float32)
    a.accumulate = int(accumulate)
    a.split_k = split_k
    a.drop_p, a.drop_seed = drop_p, drop_seed
    a.colsum = colsum.data_ptr() if colsum is not None else None
    if k_tiles is not None:
        assert k_tiles.dtype == torch.int32 and k_tiles.is_cuda and k_tiles.is_contiguous()
        a.k_tiles, a.n_k_tiles = k_tiles.data_ptr(), k_tiles.numel()
    if accumulate:
        assert out.dtype == torch.float32
        if _SPLITK_WS and split_k > 1 and nb1 * nb2 == 1 and k_tiles is None:  # opt-in: k-slices reduce through a workspace (deterministic sums)
            ws = workspace(4 * split_k * M * N, out.device, "splitk_%d" % (_raw_stream(torch.cuda.current_device()) if _raw_stream else 0))
            a.ws, a.ws_elems = ws.data_ptr(), ws.numel() // 4
    if rgrad is not None:
        coef, row_label = rgrad
        assert coef.dtype == torch.float32 and coef.is_contiguous() and row_label.dtype == torch.int32
        a.rgrad_coef, a.row_label = coef.data_ptr(), row_label.data_ptr()
    if seg is not None:  # (seg_a_off i64 device tensor, seg_b_off or None, seg_k): K-segmented operands
        a.seg_a_off, a.seg_b_off, a.seg_k = seg[0].data_ptr(), (seg[1].data_ptr() if seg[1] is not None else None), int(seg[2])
        assert seg[0].dtype == torch.int64 and seg[0].is_cuda
    if row_tiles is not None:  # i32 device tensor: the 256-row blocks of `out` to compute (tfasr_gemm_args.row_tiles; K-segmented products only)
        assert seg is not None and row_tiles.dtype == torch.int32 and row_tiles.is_cuda and row_tiles.is_contiguous()
        a.row_tiles, a.n_row_tiles = row_tiles.data_ptr(), row_tiles.numel()
    if bns is not None:
        bx, bfin, bout = bns[:3]
        bc = int(bns[3]) if len(bns) > 3 else N   # channels (the columns are (position, channel) pairs when < N)
        assert bfin.dtype == torch.float32 and bout.dtype == torch.float32 and bout.is_contiguous()
        a.bns_x, a.bns_fin, a.bns_out, a.bns_copies = bx.data_ptr(), bfin.data_ptr(), bout.data_ptr(), bout.numel() // (2 * bc)
        a.bns_c = 0 if bc == N else bc
    if lse is not None:
        part, row_label, pick = lse
        assert part.dtype == torch.float32 and pick.dtype == torch.float32 and row_label.dtype == torch.int32
        a.lse_part, a.lse_parts, a.row_label, a.pick = part.data_ptr(), part.shape[1], row_label.data_ptr(), pick.data_ptr()
    return a


def matmul(A, B, trans_a=False, trans_b=False, out=None, out_dtype=None, **kw):
    """2-D convenience: op(A)[M,K] @ op(B)[K,N]."""
    M, K = (A.shape[1], A.shape[0]) if trans_a else (A.shape[0], A.shape[1])
    N = B.shape[0] if trans_b else B.shape[1]
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype or A.dtype, device=A.device)
    return gemm(A, B, out, M, N, K, A.stride(0), B.stride(0), out.stride(0), trans_a, trans_b, **kw)


# ------------------------------------------------------------------------------------- norms
def _L():
    return _lib.load()


def layernorm_fwd(x, gamma, beta, eps=1e-3, save_stats=True):
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    check(_L().tfasr_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), rows, C, eps, _dt(x), _stream()), "layernorm_fwd")
    return y, mean, rstd


def ffn_fused_fwd(x, gamma, beta, W1, b1, W2, b2, res_factor, drop_p=0.0, seed1=0, seed2=0, save_z=True, eps=1e-3, z_factor=False):
    """tfasr_ffn_fused_fwd2: FFModule forward in one launch.  Returns (y, ln, mean, rstd, z, h), or None when the shape is outside the fused
    kernel's range (the caller keeps the layernorm + two GEMM route).  z_factor: `z` is the data gradient's factor swish'(z) * mask1 / (1 - p)
    (use it as dact_z with dact=ACT_FACTOR and no dropout term) instead of the pre-activation."""
    rows, d = x.shape
    F = W1.shape[1]
    y, ln = torch.empty_like(x), torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    z = torch.empty(rows, F, dtype=x.dtype, device=x.device) if save_z else None
    h = torch.empty(rows, F, dtype=x.dtype, device=x.device)
    st = _L().tfasr_ffn_fused_fwd2(_p(x), _p(gamma), _p(beta), _p(W1), _p(b1), _p(W2), _p(b2), _p(y), _p(ln), _p(mean), _p(rstd), _pv(z), int(bool(z_factor)),
                                   _p(h), rows, d, F, eps, float(res_factor), float(drop_p), int(seed1), int(seed2), _dt(x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "ffn_fused_fwd")
    return y, ln, mean, rstd, z, h


def ln_dense_fwd(x, gamma, beta, W, b, eps=1e-3):
    """tfasr_ln_dense_fwd: out = LayerNorm(x) W + b in one launch.  Returns (out, ln, mean, rstd) or None (shape outside the kernel's range)."""
    rows, d = x.shape
    N = W.shape[1]
    out = torch.empty(rows, N, dtype=x.dtype, device=x.device)
    ln = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    st = _L().tfasr_ln_dense_fwd(_p(x), _p(gamma), _p(beta), _p(W), _p(b), _p(out), _p(ln), _p(mean), _p(rstd), rows, d, N, eps, _dt(x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "ln_dense_fwd")
    return out, ln, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, add=None, dx=None, dropped=None, drop_p=0.0, drop_seed=0):
    """dropped (optional, same shape as dx): also receives dropout(dx, drop_p, drop_seed) from the same kernel."""
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    if dx is None:
        dx = torch.empty_like(x)
    if dropped is not None:
        check(_L().tfasr_layernorm_bwd_drop(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(add), _p(dx), _p(dgamma), _p(dbeta), _p(dropped),
                                            float(drop_p), int(drop_seed), rows, C, _dt(x), _stream()), "layernorm_bwd_drop")
        return dx
    check(_L().tfasr_layernorm_bwd(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(add), _p(dx), _p(dgamma), _p(dbeta), rows, C, _dt(x), _stream()), "layernorm_bwd")
    return dx


def layernorm_bwd_fold(dy, x, gamma, mean, rstd, dgamma, dbeta, add=None):
    """layernorm_bwd with the gamma / beta gradients through per-block partial sums + tfasr_layernorm_bwd_fold (what the native block
    executor does for the five LayerNorms of a block with ONE fold launch); returns dx, or None when the shape has no such kernel."""
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    nblk = _L().tfasr_layernorm_bwd_part_blocks(rows, C, _dt(x))
    if nblk <= 0:
        return None
    dx = torch.empty_like(x)
    part = torch.empty(nblk * 2 * C, dtype=torch.float32, device=x.device)
    check(_L().tfasr_layernorm_bwd_part(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(add), _p(dx), _p(part), None, 0.0, 0, rows, C, _dt(x),
                                        _stream()), "layernorm_bwd_part")
    dg = (ctypes.c_void_p * 1)(dgamma.data_ptr())
    db = (ctypes.c_void_p * 1)(dbeta.data_ptr())
    check(_L().tfasr_layernorm_bwd_fold(_p(part), 1, nblk, C, dg, db, _stream()), "layernorm_bwd_fold")
    return dx


def layernorm_bwd_part_n(dy, x, gamma, mean, rstd, part, nblk=None, add=None, dx=None, dropped=None, drop_p=0.0, drop_seed=0):
    """tfasr_layernorm_bwd_part_n: dx, and the gamma / beta gradients as `nblk` per-block partial sums part[nblk][2C] (slots whose block has
    no rows are zeroed).  nblk None: tfasr_layernorm_bwd_part with its own slot count, tfasr_layernorm_bwd_part_blocks(rows, C)."""
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    if dx is None:
        dx = torch.empty_like(x)
    if nblk is None:
        check(_L().tfasr_layernorm_bwd_part(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(add), _p(dx), _p(part), _p(dropped), float(drop_p),
                                            int(drop_seed), rows, C, _dt(x), _stream()), "layernorm_bwd_part")
    else:
        check(_L().tfasr_layernorm_bwd_part_n(_p(dy), _p(x), _p(gamma), _p(mean), _p(rstd), _p(add), _p(dx), _p(part), int(nblk), _p(dropped),
                                              float(drop_p), int(drop_seed), rows, C, _dt(x), _stream()), "layernorm_bwd_part_n")
    return dx


def _ptr_table(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else _p(t).value for t in ts])


def layernorm_bwd_fold_parts(part, nblk, C, dgammas, dbetas):
    """tfasr_layernorm_bwd_fold over len(dgammas) <= 8 sets that lie back to back in `part` ([nsets][nblk][2C]): dgammas[i] / dbetas[i] +=
    the column sums of set i (a None entry is skipped)."""
    check(_L().tfasr_layernorm_bwd_fold(_p(part), len(dgammas), int(nblk), int(C), _ptr_table(dgammas), _ptr_table(dbetas), _stream()),
          "layernorm_bwd_fold")


def layernorm_bwd_fold_sets(parts, nblk, C, dgammas, dbetas):
    """tfasr_layernorm_bwd_fold_sets: the same for up to 128 sets in separate buffers parts[i] ([nblk][2C] each)."""
    check(_L().tfasr_layernorm_bwd_fold_sets(_ptr_table(parts), len(parts), int(nblk), int(C), _ptr_table(dgammas), _ptr_table(dbetas), _stream()),
          "layernorm_bwd_fold_sets")


def dense_ln_bwd(dy, W, x, gamma, mean, rstd, dgamma, dbeta, add=None, dropped=None, drop_p=0.0, drop_seed=0, alpha=1.0):
    """tfasr_dense_ln_bwd: dx of `Dense(LayerNorm(x))` in one launch (dln = alpha * dy @ W^T never stored), gamma / beta gradients through
    partial sums + tfasr_layernorm_bwd_fold.  dy [rows, K], W [d, K] (the Dense kernel as stored).  Returns dx, or None when the shape is
    outside the fused kernel's range (the caller keeps gemm + layernorm_bwd)."""
    rows, d = x.numel() // x.shape[-1], x.shape[-1]
    K = dy.shape[-1]
    nblk = _L().tfasr_layernorm_bwd_part_blocks(rows, d, _dt(x))
    if nblk <= 0:
        return None
    dx = torch.empty_like(x)
    part = torch.empty(nblk * 2 * d, dtype=torch.float32, device=x.device)
    st = _L().tfasr_dense_ln_bwd(_p(dy), _p(W), K, _p(x), _p(gamma), _p(mean), _p(rstd), _p(add), _p(dx), _p(part), nblk, _p(dropped), float(drop_p),
                                 int(drop_seed), rows, d, float(alpha), _dt(x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "dense_ln_bwd")
    dg = (ctypes.c_void_p * 1)(dgamma.data_ptr())
    db = (ctypes.c_void_p * 1)(dbeta.data_ptr())
    check(_L().tfasr_layernorm_bwd_fold(_p(part), 1, nblk, d, dg, db, _stream()), "layernorm_bwd_fold")
    return dx


def bn_stats(x, stats):
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    check(_L().tfasr_bn_stats(_p(x), _p(stats), rows, C, _dt(x), _stream()), "bn_stats")


def bn_finalize(stats, count, gamma, beta, fin, moving_mean, moving_var, momentum=0.99, eps=1e-3, training=True):
    C = gamma.numel()
    check(_L().tfasr_bn_finalize(_p(stats), float(count), _p(gamma), _p(beta), _p(fin), _p(moving_mean), _p(moving_var), momentum, eps, C, int(training), _stream()), "bn_finalize")


def bn_finalize_apply_fwd(x, stats, count, gamma, beta, fin, moving_mean, moving_var, act=ACT_NONE, y=None, momentum=0.99, eps=1e-3, training=True,
                          copies=1):
    """tfasr_bn_finalize + tfasr_bn_apply_fwd in one launch (fin and the moving statistics written as bn_finalize would); returns y, or None
    when the channel count is outside the row kernel's range (the caller runs the two launches).  copies > 1: stats is [copies, 2C] (the
    layout dwconv_fwd_stats accumulates into), summed on the fly."""
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    if y is None:
        y = torch.empty_like(x)
    st = _L().tfasr_bn_finalize_apply_fwd_copies(_p(x), _p(stats), int(copies), float(count), _p(gamma), _p(beta), _p(fin), _p(moving_mean), _p(moving_var),
                                                 momentum, eps, _p(y), rows, C, act, int(training), _dt(x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "bn_finalize_apply_fwd")
    return y


def bn_apply_fwd(x, fin, act=ACT_NONE, y=None):
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    if y is None:
        y = torch.empty_like(x)
    check(_L().tfasr_bn_apply_fwd(_p(x), _p(fin), _p(y), rows, C, act, _dt(x), _stream()), "bn_apply_fwd")
    return y


def bn_bwd_stats(x, dy, fin, bstats, act=ACT_NONE):
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    check(_L().tfasr_bn_bwd_stats(_p(x), _p(dy), _p(fin), _p(bstats), rows, C, act, _dt(x), _stream()), "bn_bwd_stats")


def bn_apply_bwd(x, dy, fin, bstats, count, act=ACT_NONE, dx=None, dgamma=None, dbeta=None, grad_scale=1.0, copies=1):
    """dgamma / dbeta (f32 views of the gradient buffer): += grad_scale * the two statistics, in the same launch.  copies > 1: bstats is
    [copies, 2C] (the layout the gemm's bns epilogue accumulates into), added up on the fly."""
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    if dx is None:
        dx = torch.empty_like(x)
    check(_L().tfasr_bn_apply_bwd_grads_copies(_p(x), _p(dy), _p(fin), _p(bstats), int(copies), float(count), _p(dx), rows, C, act,
                                               _p(dgamma) if dgamma is not None else None, _p(dbeta) if dbeta is not None else None, float(grad_scale),
                                               _dt(x), _stream()), "bn_apply_bwd")
    return dx


# --------------------------------------------------------------------------------- pointwise
def cast(src, dst):
    check(_L().tfasr_cast(_p(src), _p(dst), src.numel(), _dt(src), _dt(dst), _stream()), "cast")
    return dst


def cast_colsum_many(x, y, stride, nmat, rows, C, colsums):
    """f32 matrices x + b*stride [rows, C] -> bf16 copies in y (same strides) and colsums[b] += their f32 column sums (one launch)."""
    # (the kernel takes its pointer table as an argument: at most 64 matrices per launch - a model with more blocks takes several)
    for b0 in range(0, int(nmat), 64):
        n = min(64, int(nmat) - b0)
        arr = (ctypes.c_void_p * n)(*[(t.data_ptr() if t is not None else None) for t in colsums[b0:b0 + n]])
        st = _L().tfasr_cast_colsum_many(x.data_ptr() + b0 * int(stride) * x.element_size(), y.data_ptr() + b0 * int(stride) * y.element_size(),
                                         int(stride), n, int(rows), int(C), arr, _stream())
        if st == _lib.STATUS_UNSUPPORTED:
            raise _lib.TfasrUnsupported(f"cast_colsum_many: C = {C} / stride = {stride} must be multiples of 4 and the buffers 16-byte aligned")
        check(st, "cast_colsum_many")
    return y


def dropout(x, p, seed, out=None):
    if out is None:
        out = torch.empty_like(x)
    check(_L().tfasr_dropout(_p(x), _p(out), x.numel(), p, seed, _dt(x), _stream()), "dropout")
    return out


def colsum(x2d, out, scale=1.0, rows=None, C=None, ld=None):
    rows = x2d.shape[0] if rows is None else rows
    C = x2d.shape[1] if C is None else C
    ld = x2d.stride(0) if ld is None else ld
    check(_L().tfasr_colsum(_pv(x2d), ld, _p(out), rows, C, scale, _dt(x2d), _stream()), "colsum")


def glu_fwd(x):
    rows, C2 = x.numel() // x.shape[-1], x.shape[-1]
    y = torch.empty(*x.shape[:-1], C2 // 2, dtype=x.dtype, device=x.device)
    check(_L().tfasr_glu_fwd(_p(x), _p(y), rows, C2 // 2, _dt(x), _stream()), "glu_fwd")
    return y


def glu_bwd(x, dy):
    rows, C2 = x.numel() // x.shape[-1], x.shape[-1]
    dx = torch.empty_like(x)
    check(_L().tfasr_glu_bwd(_p(x), _p(dy), _p(dx), rows, C2 // 2, _dt(x), _stream()), "glu_bwd")
    return dx


def dwconv_fwd(x, w, bias):
    B, T, C = x.shape
    y = torch.empty_like(x)
    check(_L().tfasr_dwconv_fwd(_p(x), _p(w), _p(bias), _p(y), B, T, C, w.shape[0], _dt(x), _stream()), "dwconv_fwd")
    return y


def dwconv_fwd_stats(x, w, bias, stats):
    """Depthwise conv + the BatchNorm statistics of its output in one launch: stats [copies, 2C] f32 is accumulated into (sum | sum of
    squares of the bf16-rounded outputs per channel, spread over the copies).  Returns y, or None when the fused kernel does not take the
    shape / dtype (the caller runs dwconv_fwd + bn_stats)."""
    B, T, C = x.shape
    y = torch.empty_like(x)
    st = _L().tfasr_dwconv_fwd_stats(_p(x), _p(w), _p(bias), _p(y), _p(stats), int(stats.numel() // (2 * C)), B, T, C, w.shape[0], _dt(x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "dwconv_fwd_stats")
    return y


def bn_dwconv_bwd_data_glu(bn_x, dsw, fin, bstats, count, w, glu_x, dgamma=None, dbeta=None, grad_scale=1.0):
    """BatchNorm backward apply pass (swish) + depthwise data gradient + GLU backward in one launch; bstats [copies, 2C].  Returns
    (dcv [B, T, C], dglu [B, T, 2C]) or None when the fused kernel does not take the shape."""
    B, T, C = bn_x.shape
    dcv = torch.empty_like(bn_x)
    dglu = torch.empty(B, T, 2 * C, dtype=bn_x.dtype, device=bn_x.device)
    st = _L().tfasr_bn_dwconv_bwd_data_glu(_p(bn_x), _p(dsw), _p(fin), _p(bstats), int(bstats.numel() // (2 * C)), float(count),
                                           _p(dgamma) if dgamma is not None else None, _p(dbeta) if dbeta is not None else None, float(grad_scale), _p(dcv),
                                           _p(w), _p(glu_x), _p(dglu), B, T, C, w.shape[0], _dt(bn_x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "bn_dwconv_bwd_data_glu")
    return dcv, dglu


def glu_dwconv_fwd_stats(glu_x, w, bias, stats):
    """GLU + depthwise conv + BatchNorm statistics in one launch: glu_x [B, T, 2C] -> (g [B, T, C], y [B, T, C]); stats [copies, 2C] is
    accumulated into.  None when the fused kernel does not take the shape (glu_fwd + dwconv_fwd_stats)."""
    B, T, C2 = glu_x.shape
    C = C2 // 2
    g = torch.empty(B, T, C, dtype=glu_x.dtype, device=glu_x.device)
    y = torch.empty_like(g)
    st = _L().tfasr_glu_dwconv_fwd_stats(_p(glu_x), _p(g), _p(w), _p(bias), _p(y), _p(stats), int(stats.numel() // (2 * C)), B, T, C, w.shape[0], _dt(glu_x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "glu_dwconv_fwd_stats")
    return g, y


def dwconv_bwd_data(dy, w):
    B, T, C = dy.shape
    dx = torch.empty_like(dy)
    check(_L().tfasr_dwconv_bwd_data(_p(dy), _p(w), _p(dx), B, T, C, w.shape[0], _dt(dy), _stream()), "dwconv_bwd_data")
    return dx


def dwconv_bwd_data_glu(dy, w, glu_x):
    """Depthwise data gradient + the backward of the GLU in front of the conv in one launch (bf16); None if the fused kernel does not apply."""
    B, T, C = dy.shape
    dglu = torch.empty_like(glu_x)
    st = _L().tfasr_dwconv_bwd_data_glu(_p(dy), _p(w), _p(glu_x), _p(dglu), B, T, C, w.shape[0], _dt(dy), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "dwconv_bwd_data_glu")
    return dglu


def dwconv_bwd_weight(x, dy, dw, dbias):
    B, T, C = x.shape
    n = ctypes.c_size_t(0)
    check(_L().tfasr_dwconv_bwd_weight_workspace_size(B, T, C, dw.shape[0], ctypes.byref(n)), "dwconv_bwd_weight_workspace_size")
    ws = workspace(n.value, x.device, "dwconv_wgrad_%d" % (_raw_stream(torch.cuda.current_device()) if _raw_stream else 0))
    check(_L().tfasr_dwconv_bwd_weight_ws(_p(x), _p(dy), _p(dw), _p(dbias), B, T, C, dw.shape[0], _dt(x), _p(ws), ws.numel(), _stream()),
          "dwconv_bwd_weight_ws")


def dwconv_bwd_weight_many(items):
    """Depthwise weight gradients of several layers of ONE shape as one launch pair: items = [(x [B,T,C], dy [B,T,C], dw [K,C] f32, dbias or None)]."""
    n = len(items)
    B, T, C = items[0][0].shape
    Kk = items[0][2].shape[0]
    need = ctypes.c_size_t(0)
    check(_L().tfasr_dwconv_bwd_weight_workspace_size(B, T, C, Kk, ctypes.byref(need)), "dwconv_bwd_weight_workspace_size")
    ws = workspace(n * need.value, items[0][0].device, "dw_wgrad_many")
    xa = (ctypes.c_void_p * n)(*[_p(t[0]).value for t in items])
    da = (ctypes.c_void_p * n)(*[_p(t[1]).value for t in items])
    wa = (ctypes.c_void_p * n)(*[t[2].data_ptr() for t in items])
    ba = (ctypes.c_void_p * n)(*[(t[3].data_ptr() if t[3] is not None else None) for t in items])
    check(_L().tfasr_dwconv_bwd_weight_many(xa, da, wa, ba, n, B, T, C, Kk, _dt(items[0][0]), _p(ws), ws.numel(), _stream()), "dwconv_bwd_weight_many")


def bias2_fwd(x, ldx, u, v, rows, C):
    y1 = torch.empty(rows, C, dtype=x.dtype, device=x.device)
    y2 = torch.empty(rows, C, dtype=x.dtype, device=x.device)
    check(_L().tfasr_bias2_fwd(_pv(x), ldx, _p(u), _p(v), _p(y1), _p(y2), rows, C, _dt(x), _stream()), "bias2_fwd")
    return y1, y2


def bias2_bwd(d1, d2, dx, lddx, du, dv, rows, C):
    check(_L().tfasr_bias2_bwd(_p(d1), _p(d2), _pv(dx), lddx, _p(du), _p(dv), rows, C, _dt(d1), _stream()), "bias2_bwd")


def embedding_fwd(idx, table, dtype):
    rows = idx.numel()
    V, E = table.shape
    out = torch.empty(*idx.shape, E, dtype=dtype, device=table.device)
    check(_L().tfasr_embedding_fwd(_p(idx), _p(table), _p(out), rows, E, V, _dt(out), _stream()), "embedding_fwd")
    return out


def embedding_bwd(idx, dout, dtable):
    V, E = dtable.shape
    check(_L().tfasr_embedding_bwd(_p(idx), _p(dout), _p(dtable), idx.numel(), E, V, _dt(dout), _stream()), "embedding_bwd")


def joint_fwd(enc, pred):
    B, T, J = enc.shape
    U1 = pred.shape[1]
    h = torch.empty(B, T, U1, J, dtype=enc.dtype, device=enc.device)
    check(_L().tfasr_joint_fwd(_p(enc), _p(pred), _p(h), B, T, U1, J, _dt(enc), _stream()), "joint_fwd")
    return h


def joint_bwd(h, dh):
    B, T, U1, J = h.shape
    denc = torch.empty(B, T, J, dtype=h.dtype, device=h.device)
    dpred = torch.empty(B, U1, J, dtype=h.dtype, device=h.device)
    check(_L().tfasr_joint_bwd(_p(h), _p(dh), _p(denc), _p(dpred), B, T, U1, J, _dt(h), _stream()), "joint_bwd")
    return denc, dpred


def joint_fwd_packed(enc, pred, cell_off, label_len, total_cells):
    B, T, J = enc.shape
    U1 = pred.shape[1]
    h = torch.empty(total_cells, J, dtype=enc.dtype, device=enc.device)
    check(_L().tfasr_joint_fwd_packed(_p(enc), _p(pred), _p(h), _p(cell_off), _p(label_len), total_cells, B, T, U1, J, _dt(enc), _stream()), "joint_fwd_packed")
    return h


def joint_bwd_packed(h, dh, cell_off, label_len, logit_len, B, T, U1):
    """h = None: dh already carries the tanh' factor (produced with dact=ACT_TANH_OUT)."""
    J = dh.shape[1]
    denc = torch.empty(B, T, J, dtype=dh.dtype, device=dh.device)
    dpred = torch.empty(B, U1, J, dtype=dh.dtype, device=dh.device)
    check(_L().tfasr_joint_bwd_packed(_p(h) if h is not None else None, _p(dh), _p(denc), _p(dpred), _p(cell_off), _p(label_len), _p(logit_len), B, T, U1, J, _dt(dh), _stream()), "joint_bwd_packed")
    return denc, dpred


def adam(p, g, m, v, n_reg, lr, step, beta1=0.9, beta2=0.999, eps=1e-7, weight_decay=0.0, l2=0.0, grad_scale=1.0, shadow=None):
    """shadow (bf16, p's shape): also receives the updated parameters rounded to bf16, in the same launch"""
    if shadow is not None:
        assert shadow.dtype == torch.bfloat16 and shadow.numel() == p.numel()
    check(_L().tfasr_adam_shadow(_p(p), _p(g), _p(m), _p(v), p.numel(), n_reg, lr, beta1, beta2, eps, weight_decay, l2, grad_scale, step, _p(shadow),
                                 _stream()), "adam")


def gauss_noise(x, stddev, seed):
    """x (f32, contiguous) += stddev * N(0,1), counter-based (seed, index)."""
    assert x.dtype == torch.float32 and x.is_contiguous()
    check(_L().tfasr_gauss_noise(_p(x), x.numel(), float(stddev), int(seed) & 0x7FFFFFFFFFFFFFFF, _stream()), "gauss_noise")
    return x


def axpy(y, x, alpha=1.0):
    check(_L().tfasr_axpy(_p(y), _p(x), alpha, x.numel(), _stream()), "axpy")


def sumsq(p, n, out):
    check(_L().tfasr_sumsq(_p(p), n, _p(out), _stream()), "sumsq")


def specaugment(x, fmask, tmask, mask_value=0.0):
    B, T, F = x.shape[:3]
    nf = 0 if fmask is None else fmask.shape[1]
    nt = 0 if tmask is None else tmask.shape[1]
    check(_L().tfasr_specaugment(_p(x), _p(fmask), _p(tmask), nf, nt, B, T, F, mask_value, _dt(x), _stream()), "specaugment")
    return x


# --------------------------------------------------------------------------------- attention
def relattn_softmax_fwd(content, pos, lengths, T, use_mask=True, probs=None, chunk_size=None, history_size=None):
    """content [B,H,T,ldc], pos [B,H,T,ldp] (row strides may be padded); chunk_size / history_size = streaming mask."""
    B, H, _, ldc = content.shape
    ldp = pos.shape[3]
    if probs is None:
        probs = torch.empty_like(content)
    chunk = int(chunk_size) if chunk_size else 0
    hist = int(history_size) if history_size is not None else 0
    check(_L().tfasr_relattn_softmax_fwd_streaming(_p(content), _p(pos), _p(lengths), _p(probs), B, H, T, ldc, ldp, int(use_mask), chunk, hist,
                                                   _dt(content), _stream()), "relattn_softmax_fwd")
    return probs


def relattn_softmax_bwd(probs, dprobs, lengths, T, ldp, use_mask=True, dcontent=None, dpos=None):
    B, H, _, ldc = probs.shape
    if dcontent is None:
        dcontent = torch.empty_like(probs)
    if dpos is None:
        dpos = torch.empty(B, H, T, ldp, dtype=probs.dtype, device=probs.device)
    check(_L().tfasr_relattn_softmax_bwd(_p(probs), _p(dprobs), _p(lengths), _p(dcontent), _p(dpos), B, H, T, ldc, ldp, int(use_mask), _dt(probs), _stream()), "relattn_softmax_bwd")
    return dcontent, dpos


def _window(chunk_size, history_size):
    """(chunk, hist) of the streaming attention mask for the C ABI: chunk 0 = off, hist < 0 = unlimited history"""
    if not chunk_size:
        return 0, 0
    return int(chunk_size), (-1 if history_size is None else int(history_size))


def relattn_fused_fwd(qkv, ubias, vbias, pext, lengths, B, H, T, dh, scale, use_mask=True, chunk_size=None, history_size=None):
    out = torch.empty(B * T, H * dh, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device)
    ck, hs = _window(chunk_size, history_size)
    check(_L().tfasr_relattn_fused_fwd(_p(qkv), _p(ubias), _p(vbias), _p(pext), _p(lengths), _p(out), _p(lse), B, H, T, dh, scale,
                                       int(use_mask), ck, hs, _dt(qkv), _stream()), "relattn_fused_fwd")
    return out, lse


def relattn_fused_bwd_q3(qkv, ubias, vbias, pext, lengths, o, dout, lse, dqkv, du, dv, dpext, B, H, T, dh, scale, use_mask=True, chunk_size=None,
                         history_size=None, ds=None, qv=None):
    """Query side of the fused attention backward (tfasr_relattn_fused_bwd_q3): writes dq = dqu + dqv into the q columns of dqkv
    [B*T, 3*H*dh], adds the u / v bias gradients into du / dv [H*dh] f32 and the bias row's share into dpext [2T, H*dh] f32.
    -> (ds [B,H,T,lds] unskewed score gradient, dvec [2,B,H,T], qu, qv = q + u / q + v for the key side and tfasr_relattn_dpext)."""
    lds = -(-T // 8) * 8
    if ds is None:
        ds = torch.empty(B, H, T, lds, dtype=qkv.dtype, device=qkv.device)
    dvec = torch.empty(2, B, H, T, dtype=torch.float32, device=qkv.device)  # rowsum(dout * o) | the bias-row score of every query
    qu = torch.empty(B * T, H * dh, dtype=qkv.dtype, device=qkv.device)
    if qv is None:
        qv = torch.empty(B * T, H * dh, dtype=qkv.dtype, device=qkv.device)
    check(_L().tfasr_relattn_fused_bwd_q3(_p(qkv), _p(ubias), _p(vbias), _p(pext), _p(lengths), _p(o), _p(dout), _p(lse), _p(dqkv), dqkv.stride(0),
                                          _p(du), _p(dv), _p(ds), _p(dvec), _p(dpext), _p(qu), _p(qv), B, H, T, dh, lds, scale, int(use_mask),
                                          *_window(chunk_size, history_size), _dt(qkv), _stream()), "relattn_fused_bwd_q3")
    return ds, dvec, qu, qv


def relattn_dpext(ds, qv, lengths, dpext, B, H, T, dh, use_mask=True):
    check(_L().tfasr_relattn_dpext(_p(ds), _p(qv), _p(lengths), _p(dpext), B, H, T, dh, ds.shape[3], int(use_mask), _dt(ds), _stream()), "relattn_dpext")
    return dpext


def relattn_fused_bwd_k(qkv, qu, qv, pext, lengths, dout, lse, dvec, dqkv, B, H, T, dh, scale, use_mask=True, chunk_size=None, history_size=None):
    check(_L().tfasr_relattn_fused_bwd_k(_p(qkv), _p(qu), _p(qv), _p(pext), _p(lengths), _p(dout), _p(lse), _p(dvec), _p(dqkv), B, H, T, dh,
                                         scale, int(use_mask), *_window(chunk_size, history_size), _dt(qkv), _stream()), "relattn_fused_bwd_k")
    return dqkv


def relattn_bwd_prep(qkv, ubias, vbias, pext, lengths, o, dout, B, H, T, dh, use_mask=True, qu=None, qv=None, dvec=None):
    """Preparation of the merged attention backward (tfasr_relattn_bwd_prep) -> (qu, qv [B*T, H*dh], dvec [2,B,H,T], order [B] int32:
    the samples longest first).  qu / qv / dvec may be passed in (rows of wholly padded 64-query blocks are not written)."""
    if qu is None:
        qu = torch.empty(B * T, H * dh, dtype=qkv.dtype, device=qkv.device)
    if qv is None:
        qv = torch.empty(B * T, H * dh, dtype=qkv.dtype, device=qkv.device)
    if dvec is None:
        dvec = torch.empty(2, B, H, T, dtype=torch.float32, device=qkv.device)
    order = torch.empty(B, dtype=torch.int32, device=qkv.device)
    check(_L().tfasr_relattn_bwd_prep(_p(qkv), _p(ubias), _p(vbias), _p(pext), _p(lengths), _p(o), _p(dout), _p(qu), _p(qv), _p(dvec), _p(order),
                                      B, H, T, dh, int(use_mask), _dt(qkv), _stream()), "relattn_bwd_prep")
    return qu, qv, dvec, order


def relattn_fused_bwd_qk(qkv, ubias, vbias, pext, lengths, dout, lse, qu, qv, dvec, order, dqkv, du, dv, dpext, B, H, T, dh, scale, use_mask=True,
                         chunk_size=None, history_size=None, ds=None):
    """Both sides of the fused attention backward in one launch (tfasr_relattn_fused_bwd_qk, after relattn_bwd_prep): writes dq, dk, dv
    into dqkv [B*T, 3*H*dh], adds the u / v bias gradients into du / dv and the bias row's share into dpext -> ds [B,H,T,lds]."""
    lds = -(-T // 8) * 8
    if ds is None:
        ds = torch.empty(B, H, T, lds, dtype=qkv.dtype, device=qkv.device)
    check(_L().tfasr_relattn_fused_bwd_qk(_p(qkv), _p(ubias), _p(vbias), _p(pext), _p(lengths), _p(dout), _p(lse), _p(qu), _p(qv), _p(dvec),
                                          _p(order), _p(dqkv), _p(du), _p(dv), _p(ds), _p(dpext), B, H, T, dh, lds, scale, int(use_mask),
                                          *_window(chunk_size, history_size), _dt(qkv), _stream()), "relattn_fused_bwd_qk")
    return ds


# -------------------------------------------------------------------------------------- LSTM
def lstm_step_fwd(xg_t, hr, h_prev, c_prev, lengths, t, gates_t, c_out, h_out, y_out, B, P):
    check(_L().tfasr_lstm_step_fwd(
        _pv(xg_t), xg_t.stride(0), _pv(hr), _pv(h_prev), 0 if h_prev is None else h_prev.stride(0), _pv(c_prev),
        0 if c_prev is None else c_prev.stride(0), _pv(lengths), t, _pv(gates_t), 0 if gates_t is None else gates_t.stride(0),
        _pv(c_out), c_out.stride(0), _pv(h_out), h_out.stride(0), _pv(y_out), 0 if y_out is None else y_out.stride(0), B, P,
        _dt(xg_t), _stream()), "lstm_step_fwd")


def lstm_step_bwd(dy_t, dhr, dh_carry, dc_carry, gates_t, c_t, c_prev, lengths, t, dz_t, B, P):
    check(_L().tfasr_lstm_step_bwd(
        _pv(dy_t), dy_t.stride(0), _pv(dhr), _pv(dh_carry), _pv(dc_carry), _pv(gates_t), gates_t.stride(0), _pv(c_t), c_t.stride(0),
        _pv(c_prev), 0 if c_prev is None else c_prev.stride(0), _pv(lengths), t, _pv(dz_t), dz_t.stride(0), B, P, _dt(dy_t),
        _stream()), "lstm_step_bwd")


def lstm_set_persist(mode):
    """-1: TFASR_LSTM_PERSIST from the environment, 0: per-step kernels, 1: persistent kernels; returns the previous override."""
    return int(_L().tfasr_lstm_set_persist(int(mode)))


def lstm_seq_fwd(xg, rk, h0, c0, lengths, gates, cseq, hseq, yseq, hr):
    """All U1 steps of the recurrence in one host call (contiguous [B,U1,*] buffers)."""
    B, U1, P4 = xg.shape
    P = P4 // 4
    assert xg.is_contiguous() and gates.is_contiguous() and cseq.is_contiguous() and hseq.is_contiguous() and (yseq is None or yseq.is_contiguous())
    check(_L().tfasr_lstm_seq_fwd(_p(xg), _p(rk), _pv(h0), 0 if h0 is None else h0.stride(0), _pv(c0), 0 if c0 is None else c0.stride(0), _pv(lengths),
                                  _p(gates), _p(cseq), _p(hseq), _pv(yseq), _p(hr), B, U1, P, _dt(xg), _stream()), "lstm_seq_fwd")


def lstm_seq_fwd_range(xg, rk, h0, c0, lengths, gates, cseq, hseq, yseq, hr, t0, t1):
    """steps [t0, t1) of lstm_seq_fwd with the per-step kernels (tfasr_lstm_seq_fwd_range)"""
    B, U1, P4 = xg.shape
    P = P4 // 4
    check(_L().tfasr_lstm_seq_fwd_range(_p(xg), _p(rk), _pv(h0), 0 if h0 is None else h0.stride(0), _pv(c0), 0 if c0 is None else c0.stride(0), _pv(lengths),
                                        _p(gates), _p(cseq), _p(hseq), _pv(yseq), _p(hr), B, U1, P, _dt(xg), int(t0), int(t1), _stream()),
          "lstm_seq_fwd_range")


def lstm_seq_bwd_range(dy, rk, gates, cseq, lengths, dz, dh_carry, dc_carry, dhr, t0, t1):
    """steps t1-1 .. t0 of lstm_seq_bwd with the per-step kernels (slices in descending order)"""
    B, U1, P = dy.shape
    check(_L().tfasr_lstm_seq_bwd_range(_p(dy), _p(rk), _p(gates), _p(cseq), _pv(lengths), _p(dz), _p(dh_carry), _p(dc_carry), _p(dhr), B, U1, P, _dt(dy),
                                        int(t0), int(t1), _stream()), "lstm_seq_bwd_range")


def lstm_persist_sync(device):
    """64-byte synchronisation record of the persistent LSTM kernels; word [1] != 0 after a sync = a wait timed out"""
    return torch.zeros(int(_L().tfasr_lstm_persist_sync_bytes()) // 4, dtype=torch.int32, device=device)


def lstm_persist_fwd(xg, rk, h0, c0, lengths, gates, cseq, hseq, yseq, sync):
    """tfasr_lstm_persist_fwd: the whole forward recurrence as ONE launch (raises TfasrUnsupported outside its shape range)."""
    B, U1, P4 = xg.shape
    P = P4 // 4
    assert xg.is_contiguous() and gates.is_contiguous() and cseq.is_contiguous() and hseq.is_contiguous() and (yseq is None or yseq.is_contiguous())
    check(_L().tfasr_lstm_persist_fwd(_p(xg), _p(rk), _pv(h0), 0 if h0 is None else h0.stride(0), _pv(c0), 0 if c0 is None else c0.stride(0), _pv(lengths),
                                      _p(gates), _p(cseq), _p(hseq), _pv(yseq), B, U1, P, _dt(xg), _p(sync), _stream()), "lstm_persist_fwd")


def lstm_persist_bwd(dy, rk, gates, cseq, lengths, dz, dh_carry, dc_carry, sync):
    B, U1, P = dy.shape
    assert dy.is_contiguous() and gates.is_contiguous() and cseq.is_contiguous() and dz.is_contiguous()
    check(_L().tfasr_lstm_persist_bwd(_p(dy), _p(rk), _p(gates), _p(cseq), _pv(lengths), _p(dz), _p(dh_carry), _p(dc_carry), B, U1, P, _dt(dy),
                                      _p(sync), _stream()), "lstm_persist_bwd")


def lstm_seq_bwd(dy, rk, gates, cseq, lengths, dz, dh_carry, dc_carry, dhr):
    B, U1, P = dy.shape
    assert dy.is_contiguous() and gates.is_contiguous() and cseq.is_contiguous() and dz.is_contiguous()
    check(_L().tfasr_lstm_seq_bwd(_p(dy), _p(rk), _p(gates), _p(cseq), _pv(lengths), _p(dz), _p(dh_carry), _p(dc_carry), _p(dhr), B, U1, P, _dt(dy),
                                  _stream()), "lstm_seq_bwd")


# --------------------------------------------------------------------------------- subsampling
def conv1_fwd(x, w, bias):
    B, T0, F0 = x.shape[:3]
    C = w.shape[-1]
    y = torch.empty(B, (T0 + 1) // 2, (F0 + 1) // 2, C, dtype=x.dtype, device=x.device)
    check(_L().tfasr_conv1_fwd(_p(x), _p(w), _p(bias), _p(y), B, T0, F0, C, _dt(x), _stream()), "conv1_fwd")
    return y


def conv1_bwd_weight(x, dy, dw, db):
    B, T0, F0 = x.shape[:3]
    C = dy.shape[-1]
    check(_L().tfasr_conv1_bwd_weight(_p(x), _p(dy), _p(dw), _p(db), B, T0, F0, C, _dt(x), _stream()), "conv1_bwd_weight")


# haloed space-to-depth ("S") layout helpers (include/tfasr_hip.h): y / dy are [B, T2+1, F2+1, 4, C] buffers
def conv1_fwd_s2d(x, w, bias, y):
    B, T0, F0 = x.shape[:3]
    check(_L().tfasr_conv1_fwd_s2d(_p(x), _p(w), _p(bias), _p(y), B, T0, F0, w.shape[-1], _dt(x), _stream()), "conv1_fwd_s2d")
    return y


def conv1_bwd_weight_s2d(x, dy, dw, db, C):
    B, T0, F0 = x.shape[:3]
    check(_L().tfasr_conv1_bwd_weight_s2d(_p(x), _p(dy), _p(dw), _p(db), B, T0, F0, C, _dt(x), _stream()), "conv1_bwd_weight_s2d")


def conv1_stats(x, w, bias, stats):
    B, T0, F0 = x.shape[:3]
    check(_L().tfasr_conv1_stats(_p(x), _p(w), _p(bias), _p(stats), B, T0, F0, w.shape[-1], _dt(x), _stream()), "conv1_stats")


def conv1_bn_apply_s2d(x, w, bias, fin, y):
    B, T0, F0 = x.shape[:3]
    check(_L().tfasr_conv1_bn_apply_s2d(_p(x), _p(w), _p(bias), _p(fin), _p(y), B, T0, F0, w.shape[-1], _dt(x), _stream()), "conv1_bn_apply")
    return y


def conv1_bn_bwd_stats_s2d(x, w, bias, fin, dy, bstats):
    B, T0, F0 = x.shape[:3]
    check(_L().tfasr_conv1_bn_bwd_stats_s2d(_p(x), _p(w), _p(bias), _p(fin), _p(dy), _p(bstats), B, T0, F0, w.shape[-1], _dt(x), _stream()),
          "conv1_bn_bwd_stats")


def conv1_bn_bwd_apply_s2d(x, w, bias, fin, bstats, count, dy, dw, db):
    B, T0, F0 = x.shape[:3]
    check(_L().tfasr_conv1_bn_bwd_apply_s2d(_p(x), _p(w), _p(bias), _p(fin), _p(bstats), float(count), _p(dy), _p(dw), _p(db), B, T0, F0,
                                            w.shape[-1], _dt(x), _stream()), "conv1_bn_bwd_apply")


CONV1_GRAM_DOUBLES = 768  # TFASR_CONV1_GRAM_DOUBLES (include/tfasr_hip.h)


def conv1_gram(x, gram):
    """gram: CONV1_GRAM_DOUBLES f64 (8 partial copies, stride 96, of G[9][9], s[9], N) of conv1's 3x3 patches over every output position
    of the feature map x [B, T0, F0]."""
    B, T0, F0 = x.shape[:3]
    assert gram.dtype == torch.float64 and gram.numel() >= CONV1_GRAM_DOUBLES
    check(_L().tfasr_conv1_gram(_p(x), _p(gram), B, T0, F0, _dt(x), _stream()), "conv1_gram")
    return gram


def conv1_stats_from_gram(gram, w, bias, stats):
    check(_L().tfasr_conv1_stats_from_gram(_p(gram), _p(w), _p(bias), _p(stats), w.shape[-1], _stream()), "conv1_stats_from_gram")


def conv1_bn_bwd_onepass_s2d(x, w, bias, fin, dy, bstats, pbuf, row_list=None):
    """row_list: i32 device tensor of conv1 output rows b * T1 + t, the only rows of dy that are read (None: every row)"""
    B, T0, F0 = x.shape[:3]
    assert row_list is None or (row_list.dtype == torch.int32 and row_list.is_cuda and row_list.is_contiguous())
    check(_L().tfasr_conv1_bn_bwd_onepass_s2d_rows(_p(x), _p(w), _p(bias), _p(fin), _p(dy), _p(bstats), _p(pbuf), B, T0, F0, w.shape[-1], _dt(x),
                                                   _p(row_list), 0 if row_list is None else row_list.numel(), _stream()), "conv1_bn_bwd_onepass")


def conv1_bn_bwd_finalize(gram, w, bias, fin, bstats, count, pbuf, dw, db):
    check(_L().tfasr_conv1_bn_bwd_finalize(_p(gram), _p(w), _p(bias), _p(fin), _p(bstats), float(count), _p(pbuf), _p(dw), _p(db), w.shape[-1],
                                           _stream()), "conv1_bn_bwd_finalize")


def halo_zero(x, B, T2, F2, W):
    check(_L().tfasr_halo_zero(_p(x), B, T2, F2, W, _dt(x), _stream()), "halo_zero")
    return x


def s2d_edge_zero(x, B, T1, F1, C):
    check(_L().tfasr_s2d_edge_zero(_p(x), B, T1, F1, C, _dt(x), _stream()), "s2d_edge_zero")


def s2d_tail_fill(x, tiles, rep_tt, B, T2, F2, C):
    """rows of the listed 256-row blocks of the [B, T2+1, F2+1, C] tensor x <- their utterance's representative time row (tfasr_s2d_tail_fill);
    raises TfasrUnsupported outside bf16 / C % 8 == 0."""
    assert tiles.dtype == torch.int32 and rep_tt.dtype == torch.int32 and tiles.is_cuda and rep_tt.is_cuda and rep_tt.numel() == B
    st = _L().tfasr_s2d_tail_fill(_p(x), _p(tiles), tiles.numel(), _p(rep_tt), B, T2, F2, C, _dt(x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported("s2d_tail_fill: bf16 tensors with C % 8 == 0 only")
    check(st, "s2d_tail_fill")
    return x


def s2d_tail_fold(x, r_tt, scratch, B, T2, F2, C):
    """in place on the gradient x [B, T2+1, F2+1, C]: time rows r_tt[b] .. T2 -> their f32 sum as a bf16 hi / lo pair in rows r_tt[b], r_tt[b] + 1
    and zeros behind (tfasr_s2d_tail_fold); scratch f32 [B, F2+1, C], zeroed by the caller.  Raises TfasrUnsupported outside bf16 / C % 8 == 0."""
    assert r_tt.dtype == torch.int32 and r_tt.is_cuda and r_tt.numel() == B
    assert scratch.dtype == torch.float32 and scratch.is_cuda and scratch.numel() >= B * (F2 + 1) * C
    st = _L().tfasr_s2d_tail_fold(_p(x), _p(r_tt), _p(scratch), B, T2, F2, C, _dt(x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported("s2d_tail_fold: bf16 tensors with C % 8 == 0 only")
    check(st, "s2d_tail_fold")
    return x


def im2col_3x3s2(x, col=None):
    B, T1, F1, C = x.shape
    T2, F2 = (T1 + 1) // 2, (F1 + 1) // 2
    if col is None:
        col = torch.empty(B * T2 * F2, 9 * C, dtype=x.dtype, device=x.device)
    check(_L().tfasr_im2col_3x3s2(_p(x), _p(col), B, T1, F1, C, _dt(x), _stream()), "im2col")
    return col


def col2im_3x3s2(dcol, B, T1, F1, C):
    dx = torch.empty(B, T1, F1, C, dtype=dcol.dtype, device=dcol.device)
    check(_L().tfasr_col2im_3x3s2(_p(dcol), _p(dx), B, T1, F1, C, _dt(dcol), _stream()), "col2im")
    return dx


# ------------------------------------------------------------------------------------ frontend
def logmel(signal, window, melw, band, frame_step, nfft, preemph, eps, out_dtype):
    B, N = signal.shape
    T0 = -(-N // frame_step)
    F = melw.shape[1]
    out = torch.empty(B, T0, F, dtype=out_dtype, device=signal.device)
    assert signal.dtype == torch.float32
    check(_L().tfasr_logmel(_p(signal), B, N, preemph, _p(window), window.numel(), frame_step, nfft, _p(melw), _p(band), F,
                            eps, _p(out), T0, _dt(out), _stream()), "logmel")
    return out


# -------------------------------------------------------------------------------------- greedy search
def decode_prepare(encj, nframes, frame_idx, tok_idx, active, ecur, max_tokens, mode):
    B, T, J = encj.shape
    check(_L().tfasr_decode_prepare(_p(encj), _p(nframes), _p(frame_idx), _p(tok_idx), _p(active), _p(ecur), B, T, J, max_tokens,
                                    mode, _dt(encj), _stream()), "decode_prepare")


def decode_pack(emb, lstm_k, lstm_rk, wjp, wv):
    """The f32 weights of a search step in the MFMA kernels' tile order plus G = emb @ lstm_k (csrc/decode_step.hip); None when the shapes
    have no MFMA route (the step then runs on the row-major masters).  Made once per recognize call: the weights are constants of the search."""
    V, E = emb.shape
    P = lstm_rk.shape[0]
    J = wv.shape[0]
    n = int(_L().tfasr_decode_pack_floats(E, P, J, V))
    if n == 0:
        return None
    packed = torch.empty(n, dtype=torch.float32, device=lstm_k.device)
    st = _L().tfasr_decode_pack(_p(emb), _p(lstm_k), _p(lstm_rk), _p(wjp), _p(wv), _p(packed), E, P, J, V, _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return None
    check(st, "decode_pack")
    return packed


def decode_step(emb, lstm_k, lstm_rk, lstm_b, ln_g, ln_b, wjp, bjp, wv, bv, encj, nframes, frame_idx, tok_idx, prev_tok, h, c, active, h_new, c_new,
                z, logits, max_tokens, mode, ln_eps=1e-3, packed=None):
    """Fused search step (three launches up to the f32 logits); returns False when the shapes need the per-op route."""
    B, T, J = encj.shape
    V, E = emb.shape
    P = h.shape[1]
    st = _L().tfasr_decode_step(_p(emb), _p(lstm_k), _p(lstm_rk), _p(lstm_b), _p(ln_g), _p(ln_b), _p(wjp), _p(bjp), _p(wv), _p(bv), _p(packed),
                                _p(encj), _p(nframes), _p(frame_idx), _p(tok_idx), _p(prev_tok), _p(h), _p(c), _p(active), _p(h_new), _p(c_new),
                                _p(z), _p(logits), B, T, E, P, J, V, max_tokens, mode, ln_eps, _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return False
    check(st, "decode_step")
    return True


def decode_steps(emb, lstm_k, lstm_rk, lstm_b, ln_g, ln_b, wjp, bjp, wv, bv, encj, nframes, frame_idx, tok_idx, prev_tok, h, c, active, h_new, c_new,
                 z, logits, tokens, per_frame, max_tokens, blank, mode, max_tokens_per_frame, iters, ln_eps=1e-3, packed=None):
    """`iters` fused search iterations from one host call; False when the shapes need the per-op route."""
    B, T, J = encj.shape
    V, E = emb.shape
    P = h.shape[1]
    st = _L().tfasr_decode_steps(_p(emb), _p(lstm_k), _p(lstm_rk), _p(lstm_b), _p(ln_g), _p(ln_b), _p(wjp), _p(bjp), _p(wv), _p(bv), _p(packed),
                                 _p(encj), _p(nframes), _p(frame_idx), _p(tok_idx), _p(prev_tok), _p(h), _p(c), _p(active), _p(h_new), _p(c_new),
                                 _p(z), _p(logits), _p(tokens), _p(per_frame), B, T, E, P, J, V, max_tokens, blank, mode, max_tokens_per_frame,
                                 ln_eps, int(iters), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return False
    check(st, "decode_steps")
    return True


def decode_update(logits, active, nframes, frame_idx, prev_tok, tok_idx, tokens, per_frame, h_new, c_new, h, c, max_tokens,
                  blank, mode, max_tokens_per_frame):
    B, V = logits.shape
    P = h.shape[1]
    check(_L().tfasr_decode_update(_p(logits), _p(active), _p(nframes), _p(frame_idx), _p(prev_tok), _p(tok_idx), _p(tokens),
                                   _p(per_frame), _p(h_new), _p(c_new), _p(h), _p(c), B, V, P, max_tokens, blank, mode,
                                   max_tokens_per_frame, _dt(logits), _stream()), "decode_update")


def _check_detail_buffers(what, tokens, tok_frames, tok_logp, tok_entropy):
    for t, dt in ((tok_frames, torch.int32), (tok_logp, torch.float32), (tok_entropy, torch.float32)):
        if t.dtype != dt or t.numel() != tokens.numel() or not t.is_contiguous():
            raise ValueError(f"{what}: the detail buffers are contiguous int32 / f32 / f32 tensors shaped like tokens")


def decode_update_detail(logits, active, nframes, frame_idx, prev_tok, tok_idx, tokens, per_frame, h_new, c_new, h, c, tok_frames, tok_logp,
                         tok_entropy, max_tokens, blank, mode, max_tokens_per_frame):
    """decode_update that also writes, next to every emitted symbol, its encoder frame, log-probability and the entropy of its decision into
    tok_frames (int32, caller-filled with -1) / tok_logp / tok_entropy (f32), all shaped like `tokens`."""
    B, V = logits.shape
    P = h.shape[1]
    _check_detail_buffers("decode_update_detail", tokens, tok_frames, tok_logp, tok_entropy)
    check(_L().tfasr_decode_update_detail(_p(logits), _p(active), _p(nframes), _p(frame_idx), _p(prev_tok), _p(tok_idx), _p(tokens),
                                          _p(per_frame), _p(h_new), _p(c_new), _p(h), _p(c), _p(tok_frames), _p(tok_logp), _p(tok_entropy),
                                          B, V, P, max_tokens, blank, mode, max_tokens_per_frame, _dt(logits), _stream()), "decode_update_detail")


def decode_steps_detail(emb, lstm_k, lstm_rk, lstm_b, ln_g, ln_b, wjp, bjp, wv, bv, encj, nframes, frame_idx, tok_idx, prev_tok, h, c, active,
                        h_new, c_new, z, logits, tokens, per_frame, tok_frames, tok_logp, tok_entropy, max_tokens, blank, mode,
                        max_tokens_per_frame, iters, ln_eps=1e-3, packed=None):
    """decode_steps with the detail bookkeeping of decode_update_detail; False when the shapes need the per-op route."""
    B, T, J = encj.shape
    V, E = emb.shape
    P = h.shape[1]
    _check_detail_buffers("decode_steps_detail", tokens, tok_frames, tok_logp, tok_entropy)
    st = _L().tfasr_decode_steps_detail(_p(emb), _p(lstm_k), _p(lstm_rk), _p(lstm_b), _p(ln_g), _p(ln_b), _p(wjp), _p(bjp), _p(wv), _p(bv),
                                        _p(packed), _p(encj), _p(nframes), _p(frame_idx), _p(tok_idx), _p(prev_tok), _p(h), _p(c), _p(active),
                                        _p(h_new), _p(c_new), _p(z), _p(logits), _p(tokens), _p(per_frame), _p(tok_frames), _p(tok_logp),
                                        _p(tok_entropy), B, T, E, P, J, V, max_tokens, blank, mode, max_tokens_per_frame, ln_eps, int(iters),
                                        _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        return False
    check(st, "decode_steps_detail")
    return True


# ------------------------------------------------------------------------------------------------ CTC
def ctc_loss_fwd_bwd(logits, labels, label_len, logit_len, grad_scale=None, grads=None, want_grads=True, blank=0):
    """logits [B,T,V] -> (costs [B], grads or None); tf.nn.ctc_loss semantics (losses/ctc_loss.py:57-66)."""
    B, T, V = logits.shape
    U = labels.shape[1]
    # kernel limits (one lattice state per thread, per-class occupancy in LDS): say so instead of a bare INVALID_VALUE
    if 2 * U + 1 > 1024:
        raise ValueError(f"tfasr_ctc_loss: padded label length {U} > 511 (2U+1 lattice states must fit one 1024-thread workgroup); crop the label padding")
    if V * 4 > 64 * 1024:
        raise ValueError(f"tfasr_ctc_loss: vocabulary {V} > 16384 classes (the per-class occupancy buffer of the gradient kernel lives in LDS)")
    costs = torch.empty(B, dtype=torch.float32, device=logits.device)
    if want_grads and grads is None:
        grads = torch.empty_like(logits)
    n = ctypes.c_size_t(0)
    check(_L().tfasr_ctc_loss_workspace_size(B, T, U, V, ctypes.byref(n)), "ctc_ws")
    ws = workspace(n.value, logits.device, "ctc")
    check(_L().tfasr_ctc_loss(_p(logits), _p(grads) if want_grads else None, _p(labels), _p(label_len), _p(logit_len), _p(grad_scale),
                              B, T, U, V, blank, _dt(logits), _p(costs), _p(ws), ws.numel(), _stream()), "ctc_loss")
    return costs, (grads if want_grads else None)


def ctc_beam_search(logits, logit_len, beam_width=10, blank_index=None):
    """tf.nn.ctc_beam_search_decoder semantics (top path, dense, 0 padded).  Host routine (as in the reference): the logits
    are copied to host memory.  blank_index=None reproduces the reference call (TF convention: the LAST class is blank)."""
    import numpy as np

    x = logits.detach().float().cpu().contiguous().numpy()
    B, T, V = x.shape
    ln = np.ascontiguousarray(logit_len.detach().cpu().numpy() if hasattr(logit_len, "detach") else logit_len, dtype=np.int32)
    toks = np.zeros((B, T), np.int32)
    n = np.zeros(B, np.int32)
    lp = np.zeros(B, np.float32)
    bi = V - 1 if blank_index is None else int(blank_index)
    check(_L().tfasr_ctc_beam_search_host(x.ctypes.data, ln.ctypes.data, B, T, V, int(beam_width), bi, toks.ctypes.data, n.ctypes.data,
                                          lp.ctypes.data), "ctc_beam_search")
    return torch.from_numpy(toks), torch.from_numpy(n), torch.from_numpy(lp)


def _beam_args(what, V, beam_width, top_paths, blank, blank_name="blank"):
    """The checks of every device beam search entry point `what`, before anything is queued -> (beam_width, top_paths, blank) as
    ints."""
    beam_width, top_paths, blank = int(beam_width), int(top_paths), int(blank)
    if not 1 <= beam_width <= 64:
        raise ValueError(f"{what}: beam_width {beam_width} outside [1, 64] (a beam lives in one workgroup's LDS)")
    if not 1 <= top_paths <= beam_width:
        raise ValueError(f"{what}: top_paths {top_paths} outside [1, beam_width = {beam_width}]")
    if V < 2 or not 0 <= blank < V:
        raise ValueError(f"{what}: {blank_name} {blank} outside [0, V = {V}) or V < 2")
    return beam_width, top_paths, blank


def _paths(B, P, L, dev):
    """what an n-best list is returned in: tokens [B, P, L] int32, lengths [B, P] int32, scores [B, P] f32"""
    return (torch.empty(B, P, L, dtype=torch.int32, device=dev), torch.empty(B, P, dtype=torch.int32, device=dev),
            torch.empty(B, P, dtype=torch.float32, device=dev))


def ctc_beam_search_device(logits, logit_len, beam_width=10, top_paths=1, blank_index=None):
    """The prefix beam search of ctc_beam_search on the device (tfasr_ctc_beam_search), stream ordered, with the n-best list:
    logits [B,T,V] f32 / bf16 on the GPU, logit_len [B] -> device tensors tokens [B,P,T] (0 padded), lengths [B,P], log_prob [B,P],
    best first; paths past the last live beam are empty with log_prob -inf.  blank_index=None: class V-1 (TF's convention)."""
    B, T, V = logits.shape
    bi = V - 1 if blank_index is None else blank_index
    beam_width, top_paths, bi = _beam_args("tfasr_ctc_beam_search", V, beam_width, top_paths, bi, "blank_index")
    logits = logits.contiguous()
    dev = logits.device
    if not torch.is_tensor(logit_len):
        logit_len = torch.tensor(logit_len, dtype=torch.int32)
    logit_len = logit_len.to(device=dev, dtype=torch.int32).contiguous()
    n = ctypes.c_size_t(0)
    check(_L().tfasr_ctc_beam_search_workspace_size(B, T, V, beam_width, ctypes.byref(n)), "ctc_beam_ws")
    ws = workspace(n.value, dev, "ctc_beam")
    tokens, lengths, log_prob = _paths(B, top_paths, T, dev)
    check(_L().tfasr_ctc_beam_search(_p(logits), _p(logit_len), B, T, V, beam_width, top_paths, bi, _dt(logits), _p(tokens), _p(lengths),
                                     _p(log_prob), _p(ws), ws.numel(), _stream()), "ctc_beam_search_device")
    return tokens, lengths, log_prob


CTC_LM_MAX_BEAM = 32  # TFASR_CTC_LM_MAX_BEAM


class NGramLmStruct(ctypes.Structure):  # tfasr_ngram_lm_t
    _fields_ = [("keys", ctypes.c_void_p), ("vals", ctypes.c_void_p), ("wlogp", ctypes.c_void_p), ("wbow", ctypes.c_void_p),
                ("weos", ctypes.c_void_p), ("suffix", ctypes.c_void_p), ("depth", ctypes.c_void_p),
                ("nodes", ctypes.c_int32), ("table_size", ctypes.c_int32), ("order", ctypes.c_int32), ("start", ctypes.c_int32),
                ("eos", ctypes.c_int32)]


_LM_ARRAYS = ("keys", "vals", "wlogp", "wbow", "weos", "suffix", "depth")


def _lm_struct(t, ptrs):
    return NGramLmStruct(*ptrs, t.nodes, t.table_size, t.order, t.start, t.eos)


def _lm_host(t):
    """tfasr_ngram_lm_t over the NumPy arrays of lm.NGramTables"""
    if t._struct is None:
        t._struct = _lm_struct(t, [getattr(t, a).ctypes.data for a in _LM_ARRAYS])
    return t._struct


def _lm_device(t, dev):
    """the same over device copies, uploaded once per (tables, device); the tables are cached per (alpha, beta) by the NGramLM"""
    key = str(dev)
    if key not in t._device:
        import numpy as np

        tens = [torch.from_numpy(getattr(t, a).view(np.int64) if a == "keys" else getattr(t, a)).to(dev) for a in _LM_ARRAYS]
        t._device[key] = (tens, _lm_struct(t, [x.data_ptr() for x in tens]))
    return t._device[key][1]


def _lm_beam_args(what, V, beam_width, top_paths, blank, lm_tables):
    if int(lm_tables.vocab_size) != int(V) or int(lm_tables.blank) != int(blank):
        raise ValueError(f"{what}: the language model was built for vocab_size {lm_tables.vocab_size} with blank {lm_tables.blank}, the "
                         f"logits have V = {V} with blank_index {int(blank)} (another vocabulary would score <s> / </s> or a missing "
                         "unigram as a class)")
    if not 1 <= int(beam_width) <= CTC_LM_MAX_BEAM:
        raise ValueError(f"{what}: beam_width {int(beam_width)} outside [1, {CTC_LM_MAX_BEAM}] (the fused candidate list of a frame, "
                         f"3W + W * min(2W, V-1) entries, lives in one workgroup's LDS)")
    return _beam_args(what, V, beam_width, top_paths, blank, "blank_index")


def ctc_beam_search_lm_host(logits, logit_len, lm_tables, beam_width=10, top_paths=1, blank_index=0):
    """The prefix beam search with an n-gram LM fused in, host routine (tfasr_ctc_beam_search_lm_host): maximises log P_ctc(y | x) +
    lm(y).  lm_tables = NGramLM.tables(alpha, beta).  -> CPU tensors tokens [B,P,T] (0 padded), lengths [B,P], score [B,P], log_prob
    [B,P] (the acoustic total), lm_score [B,P] (lm + the end-of-sentence term), best first by score = log_prob + lm_score; paths past
    the last live beam are empty with score = log_prob = -inf.  Per frame only the min(2W, V-1) acoustically best non-blank classes
    extend a row (the device search's pruning, part of the decoder's definition).  blank_index is the model's blank (default 0)."""
    import numpy as np

    x = logits.detach().float().cpu().contiguous().numpy()
    B, T, V = x.shape
    W, P, bi = _lm_beam_args("tfasr_ctc_beam_search_lm_host", V, beam_width, top_paths, blank_index, lm_tables)
    ln = np.ascontiguousarray(logit_len.detach().cpu().numpy() if hasattr(logit_len, "detach") else logit_len, dtype=np.int32)
    toks, n = np.zeros((B, P, T), np.int32), np.zeros((B, P), np.int32)
    sc, lp, ls = np.zeros((B, P), np.float32), np.zeros((B, P), np.float32), np.zeros((B, P), np.float32)
    st = _lm_host(lm_tables)
    check(_L().tfasr_ctc_beam_search_lm_host(x.ctypes.data, ln.ctypes.data, B, T, V, W, P, bi, ctypes.addressof(st), toks.ctypes.data,
                                             n.ctypes.data, sc.ctypes.data, lp.ctypes.data, ls.ctypes.data), "ctc_beam_search_lm_host")
    return tuple(torch.from_numpy(a) for a in (toks, n, sc, lp, ls))


def ctc_beam_search_lm(logits, logit_len, lm_tables, beam_width=10, top_paths=1, blank_index=0):
    """ctc_beam_search_lm_host on the device (tfasr_ctc_beam_search_lm), stream ordered: logits [B,T,V] f32 / bf16 on the GPU ->
    device tensors tokens [B,P,T], lengths [B,P], score [B,P], log_prob [B,P], lm_score [B,P], best first.  1 <= beam_width <= 32.
    With alpha = beta = 0 the tokens, lengths and log_prob are those of ctc_beam_search_device, bit for bit."""
    B, T, V = logits.shape
    W, P, bi = _lm_beam_args("tfasr_ctc_beam_search_lm", V, beam_width, top_paths, blank_index, lm_tables)
    logits = logits.contiguous()
    dev = logits.device
    logit_len = _i32(logit_len, dev)
    st = _lm_device(lm_tables, dev)
    n = ctypes.c_size_t(0)
    check(_L().tfasr_ctc_beam_search_lm_workspace_size(B, T, V, W, ctypes.byref(n)), "ctc_beam_lm_ws")
    ws = workspace(n.value, dev, "ctc_beam_lm")
    tokens, lengths, score = _paths(B, P, T, dev)
    log_prob, lm_score = torch.empty_like(score), torch.empty_like(score)
    check(_L().tfasr_ctc_beam_search_lm(_p(logits), _p(logit_len), B, T, V, W, P, bi, _dt(logits), ctypes.addressof(st), _p(tokens),
                                        _p(lengths), _p(score), _p(log_prob), _p(lm_score), _p(ws), ws.numel(), _stream()),
          "ctc_beam_search_lm")
    return tokens, lengths, score, log_prob, lm_score


def _i32(x, dev):
    if not torch.is_tensor(x):
        x = torch.tensor(x, dtype=torch.int32)
    return x.to(device=dev, dtype=torch.int32).contiguous()


def rnnt_beam_workspace_size(B, T, U, J, V, beam_width):
    n = ctypes.c_size_t(0)
    check(_L().tfasr_rnnt_beam_workspace_size(B, T, U, J, V, int(beam_width), ctypes.byref(n)), "rnnt_beam_ws")
    return n.value


def rnnt_beam_search(emb, lstm_k, lstm_rk, lstm_b, ln_g, ln_b, wjp, bjp, wv, bv, encj, nframes, beam_width=10, top_paths=1, blank=0,
                     init_tok=None, init_h=None, init_c=None, ln_eps=1e-3, packed=None):
    """Transducer modified beam search (tfasr_rnnt_beam_search), the whole search queued by one call: f32 weights as decode_step takes
    them, encj [B,T,J] f32, nframes [B] (<= T) -> device tensors tokens [B,NP,T] (blank padded), lengths [B,NP], scores [B,NP] f32,
    next_tok [B,NP], next_h / next_c [B,NP,U], best first; paths past the last live hypothesis are empty with score -inf."""
    B, T, J = encj.shape
    V, E = emb.shape
    U = lstm_rk.shape[0]
    beam_width, top_paths, blank = _beam_args("tfasr_rnnt_beam_search", V, beam_width, top_paths, blank)
    dev = encj.device
    nframes = _i32(nframes, dev)
    if init_tok is not None:
        init_tok = _i32(init_tok, dev).reshape(B)
    ws = workspace(rnnt_beam_workspace_size(B, T, U, J, V, beam_width), dev, "rnnt_beam")
    tokens, lengths, scores = _paths(B, top_paths, T, dev)
    next_tok = torch.empty(B, top_paths, dtype=torch.int32, device=dev)
    next_h = torch.empty(B, top_paths, U, dtype=torch.float32, device=dev)
    next_c = torch.empty(B, top_paths, U, dtype=torch.float32, device=dev)
    check(_L().tfasr_rnnt_beam_search(_p(emb), _p(lstm_k), _p(lstm_rk), _p(lstm_b), _p(ln_g), _p(ln_b), _p(wjp), _p(bjp), _p(wv), _p(bv),
                                      _p(packed), _p(encj), _p(nframes), _p(init_tok), _p(init_h), _p(init_c), B, T, E, U, J, V, beam_width,
                                      top_paths, blank, ln_eps, _p(tokens), _p(lengths), _p(scores), _p(next_tok), _p(next_h), _p(next_c),
                                      _p(ws), ws.numel(), _stream()), "rnnt_beam_search")
    return tokens, lengths, scores, next_tok, next_h, next_c


class RnntBeamSeam:
    """A beam search driven from outside (tfasr_rnnt_beam_begin / _select / _nbest): the caller supplies the logits of every frame,
    which is how a test replaces the joint network by a model of its own."""

    def __init__(self, B, T, V, beam_width, blank=0, init_tok=None, device="cuda"):
        self.beam_width, _, self.blank = _beam_args("tfasr_rnnt_beam_search", V, beam_width, 1, blank)
        self.B, self.T, self.V, self.U, self.J = int(B), int(T), int(V), 1, 1
        self.ws = torch.empty(rnnt_beam_workspace_size(self.B, self.T, 1, 1, self.V, self.beam_width), dtype=torch.uint8, device=device)
        tok = None if init_tok is None else _i32(init_tok, self.ws.device)
        check(_L().tfasr_rnnt_beam_begin(_p(tok), self.B, self.T, 1, 1, self.V, self.beam_width, self.blank, _p(self.ws), self.ws.numel(),
                                         _stream()), "rnnt_beam_begin")

    def select(self, logits, nframes, t):
        """one frame t from logits [B, beam_width, V] f32 of the current beam rows"""
        logits = logits.to(self.ws.device, torch.float32).contiguous()
        if tuple(logits.shape) != (self.B, self.beam_width, self.V):
            raise ValueError(f"rnnt_beam_select: logits {tuple(logits.shape)}, expected {(self.B, self.beam_width, self.V)}")
        check(_L().tfasr_rnnt_beam_select(_p(logits), _p(_i32(nframes, self.ws.device)), int(t), self.B, self.T, self.U, self.J, self.V,
                                          self.beam_width, self.blank, _p(self.ws), self.ws.numel(), _stream()), "rnnt_beam_select")

    def nbest(self, top_paths=None):
        """the best top_paths rows (default: all) -> tokens [B,NP,T], lengths [B,NP], scores [B,NP]"""
        _, top_paths, _ = _beam_args("tfasr_rnnt_beam_search", self.V, self.beam_width, top_paths or self.beam_width, self.blank)
        dev = self.ws.device
        tokens, lengths, scores = _paths(self.B, top_paths, self.T, dev)
        check(_L().tfasr_rnnt_beam_nbest(self.B, self.T, self.U, self.J, self.V, self.beam_width, top_paths, self.blank, _p(tokens),
                                         _p(lengths), _p(scores), _p(self.ws), self.ws.numel(), _stream()), "rnnt_beam_nbest")
        return tokens, lengths, scores


def rnnt_beam_begin(B, T, V, beam_width, blank=0, init_tok=None, device="cuda"):
    return RnntBeamSeam(B, T, V, beam_width, blank, init_tok, device)


def rnnt_beam_select(seam, logits, nframes, t):
    seam.select(logits, nframes, t)


def rnnt_beam_nbest(seam, top_paths=None):
    return seam.nbest(top_paths)


MAX_HORIZON = 4096  # TFASR_BEAM_MAX_HORIZON


def _row_mask(rows, B, dev):
    """rows (None = all) -> [B] int32 device mask, or None"""
    if rows is None:
        return None
    rows = [int(b) for b in rows]
    if any(not 0 <= b < B for b in rows):
        raise ValueError(f"stream rows {rows} outside [0, B = {B})")
    m = torch.zeros(B, dtype=torch.int32)
    if rows:
        m[rows] = 1
    return m.to(dev)


class _BeamStream:
    """What RnntBeamStream and CtcBeamStream share: the host's frame counts (the capacity check needs no device round trip), the
    committed depths, the commit calls and the compaction.

    commit(horizon=H) prunes as well as commits (tfasr_*_beam_commit_horizon); its per-stream horizon state is made at the
    first such call, and one object keeps one H.  compact() sheds the trie above and beside the live rows; after it `frames` counts the
    frames a stream's trie still answers for (the depth of its deepest live row), nbest() returns the label sequences below the new
    root, and dropped[b] holds the labels in front of them."""

    def _init_common(self, B, Tcap, V, beam_width, device):
        self.B, self.Tcap, self.V = int(B), int(Tcap), int(V)
        if self.B < 1 or self.Tcap < 1:
            raise ValueError(f"{self.what}: B {self.B} and Tcap {self.Tcap} must be >= 1")
        self.frames = [0] * self.B  # frames per stream since its reset (or, after a compaction, the depth of its deepest live row)
        self.committed = torch.zeros(self.B, dtype=torch.int32, device=device)
        self.horizon, self.hstate = None, None  # commit(horizon=H): H, and the [B, 4 + 2 (H + 1)] int32 state the kernels keep
        self.dropped = [[] for _ in range(self.B)]  # the labels compact() has taken out of each stream's trie

    def _take(self, nvalid, C):
        """check a chunk's nvalid (host values) against C and the capacity BEFORE anything is queued -> (list, frames_max_after)"""
        nv = [int(v) for v in (nvalid.tolist() if hasattr(nvalid, "tolist") else nvalid)]
        if len(nv) != self.B or any(not 0 <= v <= C for v in nv):
            raise ValueError(f"{self.what}: nvalid {nv} must be [B = {self.B}] values in [0, C = {C}]")
        after = [f + v for f, v in zip(self.frames, nv)]
        for b, a in enumerate(after):
            if a > self.Tcap:
                raise RuntimeError(f"{self.what}: stream {b} would reach {a} frames, past its capacity of {self.Tcap}: reset it")
        return nv, max(after)

    def _reset_host(self, rows):
        for b in (range(self.B) if rows is None else rows):
            self.frames[int(b)] = 0
            self.dropped[int(b)] = []
        if rows is None:
            self.committed.zero_()
            if self.hstate is not None:
                self.hstate.zero_()
        elif len(rows):
            r = torch.as_tensor([int(b) for b in rows], dtype=torch.long, device=self.committed.device)
            self.committed[r] = 0
            if self.hstate is not None:
                self.hstate[r] = 0

    def _width(self):
        return max(max(self.frames), 1)  # a hypothesis is never longer than the frames consumed

    def commit(self, final_rows=(), horizon=None):
        """-> (tokens [B, width] padded with the search's pad value (transducer: blank, CTC: 0), ntokens [B]) device tensors: the
        labels new in the streams' stable prefixes (the part every live hypothesis shares); the streams in final_rows commit their
        whole best hypothesis.  horizon=H (encoder frames, >= 1): a stream that has consumed frames since the previous call also drops
        the rows that disagree with what its best row held H frames ago, and commits up to there."""
        dev, width = self.ws.device, self._width()
        final_rows = list(final_rows)
        if horizon is not None:
            self._horizon_state(horizon)
        fin = _row_mask(final_rows, self.B, dev) if final_rows else None
        tokens = torch.empty(self.B, width, dtype=torch.int32, device=dev)
        n = torch.empty(self.B, dtype=torch.int32, device=dev)
        if horizon is None:
            self._commit(_p(fin), _p(tokens), _p(n), width)
        else:
            self._commit_horizon(_p(fin), _p(tokens), _p(n), width)
        return tokens, n

    def _horizon_state(self, horizon):
        horizon = int(horizon)
        if not 1 <= horizon <= MAX_HORIZON:
            raise ValueError(f"{self.what}: horizon {horizon} outside [1, {MAX_HORIZON}] encoder frames")
        if self.horizon is None:
            self.horizon = horizon
            self.hstate = torch.zeros(self.B, 4 + 2 * (horizon + 1), dtype=torch.int32, device=self.ws.device)
        elif horizon != self.horizon:
            raise ValueError(f"{self.what}: this stream object runs horizon {self.horizon}, not {horizon} (its prune-point ring has that size)")

    def compact(self, rows=None):
        """Shed the trie nodes above and beside the live rows of the given streams (default: all), in place -> per stream the list
        [labels dropped from the front, trie nodes kept, frames]: `frames` (also self.frames[b]) is the depth of the deepest live row,
        what the capacity check counts from now on.  The dropped labels are committed ones and go to self.dropped[b].  One
        device-to-host read."""
        dev = self.ws.device
        mask = _row_mask(range(self.B) if rows is None else list(rows), self.B, dev)
        head = self.nbest(1)[0][:, 0, :]  # the labels in front of the new root are the first ones of every live row
        out = torch.empty(self.B, 3, dtype=torch.int32, device=dev)
        self._compact(_p(mask), _p(self.hstate), self.horizon or 0, _p(out))
        host = torch.cat([out, head], 1).cpu()
        res = host[:, :3].tolist()
        for b, (drop, _, frames) in enumerate(res):
            self.dropped[b] += host[b, 3:3 + drop].tolist()
            self.frames[b] = frames
        return res


class RnntBeamStream(_BeamStream):
    """The transducer beam search in pieces (tfasr_rnnt_beam_reset / _advance / _commit / _nbest_states): B streams, each carrying its
    whole beam from chunk to chunk in a workspace this object owns (never the cached workspace() of the one-shot search).  weights =
    (emb, lstm_k, lstm_rk, lstm_b, ln_g, ln_b, wjp, bjp, wv, bv) f32, as rnnt_beam_search takes them.  Tcap = the most frames a stream
    consumes between resets."""
    what = "tfasr_rnnt_beam_advance"

    def __init__(self, weights, B, Tcap, beam_width, blank=0, ln_eps=1e-3, packed=None):
        emb, lstm_k, lstm_rk, lstm_b, ln_g, ln_b, wjp, bjp, wv, bv = weights
        self.weights, self.packed, self.ln_eps = tuple(weights), packed, float(ln_eps)
        V, self.E = emb.shape
        self.U, self.J = lstm_rk.shape[0], wjp.shape[1]
        self.beam_width, _, self.blank = _beam_args("tfasr_rnnt_beam_search", V, beam_width, 1, blank)
        self._init_common(B, Tcap, V, beam_width, emb.device)
        self.ws = torch.empty(rnnt_beam_workspace_size(self.B, self.Tcap, self.U, self.J, self.V, self.beam_width), dtype=torch.uint8,
                              device=emb.device)
        self.reset()

    def _dims(self):
        return self.B, self.Tcap, self.U, self.J, self.V, self.beam_width

    def reset(self, rows=None):
        """one empty hypothesis for the given streams (default: all); the others keep every bit"""
        rows = None if rows is None else list(rows)
        mask = _row_mask(rows, self.B, self.ws.device)
        check(_L().tfasr_rnnt_beam_reset(_p(mask), *self._dims(), self.blank, _p(self.ws), self.ws.numel(), _stream()), "rnnt_beam_reset")
        self._reset_host(rows)

    def advance(self, encj, nvalid):
        """encj [B, C, J] f32 (device), nvalid [B] host values in [0, C]: frame t is searched for the streams with t < nvalid[b]"""
        if encj.dim() != 3 or encj.shape[0] != self.B or encj.shape[2] != self.J or encj.dtype != torch.float32:
            raise ValueError(f"rnnt_beam_advance: encj {tuple(encj.shape)} {encj.dtype}, expected [{self.B}, C, {self.J}] float32")
        C = int(encj.shape[1])
        nv, after = self._take(nvalid, C)
        encj = encj.contiguous()
        w = self.weights
        check(_L().tfasr_rnnt_beam_advance(*[_p(x) for x in w], _p(self.packed), _p(encj), _p(_i32(nv, self.ws.device)), self.B, C,
                                           self.Tcap, self.E, self.U, self.J, self.V, self.beam_width, self.blank, self.ln_eps, after,
                                           _p(self.ws), self.ws.numel(), _stream()), "rnnt_beam_advance")
        self.frames = [f + v for f, v in zip(self.frames, nv)]

    def _commit(self, fin, tokens, n, width):
        check(_L().tfasr_rnnt_beam_commit(fin, _p(self.committed), tokens, n, *self._dims(), width, self.blank, _p(self.ws),
                                          self.ws.numel(), _stream()), "rnnt_beam_commit")

    def _commit_horizon(self, fin, tokens, n, width):
        check(_L().tfasr_rnnt_beam_commit_horizon(fin, _p(self.committed), tokens, n, _p(self.hstate), self.horizon, *self._dims(), width,
                                                  self.blank, _p(self.ws), self.ws.numel(), _stream()), "rnnt_beam_commit_horizon")

    def _compact(self, mask, hstate, horizon, out):
        check(_L().tfasr_rnnt_beam_compact(mask, _p(self.committed), hstate, horizon, out, *self._dims(), _p(self.ws), self.ws.numel(),
                                           _stream()), "rnnt_beam_compact")

    def nbest(self, top_paths=None):
        """the current beams as rnnt_beam_search returns them: (tokens [B, NP, L], lengths, scores, next_tok, next_h, next_c), L = the
        most frames a stream has consumed (at least 1)"""
        _, top_paths, _ = _beam_args("tfasr_rnnt_beam_search", self.V, self.beam_width, top_paths or self.beam_width, self.blank)
        dev, width, B, U = self.ws.device, self._width(), self.B, self.U
        tokens, lengths, scores = _paths(B, top_paths, width, dev)
        next_tok = torch.empty(B, top_paths, dtype=torch.int32, device=dev)
        next_h = torch.empty(B, top_paths, U, dtype=torch.float32, device=dev)
        next_c = torch.empty(B, top_paths, U, dtype=torch.float32, device=dev)
        check(_L().tfasr_rnnt_beam_nbest_states(*self._dims(), top_paths, self.blank, width, _p(tokens), _p(lengths), _p(scores),
                                                _p(next_tok), _p(next_h), _p(next_c), _p(self.ws), self.ws.numel(), _stream()),
              "rnnt_beam_nbest_states")
        return tokens, lengths, scores, next_tok, next_h, next_c


class CtcBeamStream(_BeamStream):
    """The CTC prefix beam search in pieces (tfasr_ctc_beam_reset / _advance / _commit / _nbest): B streams, chunks of at most C
    frames, at most Tcap frames per stream between resets; the workspace (this object's own) carries the beams.  blank_index=None: class
    V-1, as ctc_beam_search_device."""
    what = "tfasr_ctc_beam_advance"

    def __init__(self, B, C, Tcap, V, beam_width, blank_index=None, device="cuda"):
        self.C = int(C)
        bi = int(V) - 1 if blank_index is None else blank_index
        self.beam_width, _, self.blank_index = _beam_args("tfasr_ctc_beam_advance", V, beam_width, 1, bi, "blank_index")
        if not 1 <= self.C <= int(Tcap):
            raise ValueError(f"tfasr_ctc_beam_advance: chunk capacity {self.C} outside [1, Tcap = {Tcap}]")
        self._init_common(B, Tcap, V, beam_width, device)
        n = ctypes.c_size_t(0)
        check(_L().tfasr_ctc_beam_stream_workspace_size(*self._dims(), ctypes.byref(n)), "ctc_beam_stream_ws")
        self.ws = torch.empty(n.value, dtype=torch.uint8, device=device)
        self.reset()

    def _dims(self):
        return self.B, self.C, self.Tcap, self.V, self.beam_width

    def reset(self, rows=None):
        rows = None if rows is None else list(rows)
        mask = _row_mask(rows, self.B, self.ws.device)
        check(_L().tfasr_ctc_beam_reset(_p(mask), *self._dims(), _p(self.ws), self.ws.numel(), _stream()), "ctc_beam_reset")
        self._reset_host(rows)

    def advance(self, logits, nvalid):
        """logits [B, Cn <= C, V] f32 / bf16 (device), nvalid [B] host values in [0, Cn]"""
        if logits.dim() != 3 or logits.shape[0] != self.B or logits.shape[2] != self.V or not 1 <= logits.shape[1] <= self.C:
            raise ValueError(f"ctc_beam_advance: logits {tuple(logits.shape)}, expected [{self.B}, <= {self.C}, {self.V}]")
        Cn = int(logits.shape[1])
        nv, after = self._take(nvalid, Cn)
        logits = logits.contiguous()
        B, C, Tcap, V, W = self._dims()
        check(_L().tfasr_ctc_beam_advance(_p(logits), _p(_i32(nv, self.ws.device)), B, C, Cn, Tcap, V, W, self.blank_index, _dt(logits),
                                          after, _p(self.ws), self.ws.numel(), _stream()), "ctc_beam_advance")
        self.frames = [f + v for f, v in zip(self.frames, nv)]

    def _commit(self, fin, tokens, n, width):
        check(_L().tfasr_ctc_beam_commit(fin, _p(self.committed), tokens, n, *self._dims(), width, _p(self.ws), self.ws.numel(),
                                         _stream()), "ctc_beam_commit")

    def _commit_horizon(self, fin, tokens, n, width):
        check(_L().tfasr_ctc_beam_commit_horizon(fin, _p(self.committed), tokens, n, _p(self.hstate), self.horizon, *self._dims(), width,
                                                 _p(self.ws), self.ws.numel(), _stream()), "ctc_beam_commit_horizon")

    def _compact(self, mask, hstate, horizon, out):
        check(_L().tfasr_ctc_beam_compact(mask, _p(self.committed), hstate, horizon, out, *self._dims(), _p(self.ws), self.ws.numel(),
                                          _stream()), "ctc_beam_compact")

    def nbest(self, top_paths=None):
        """the current beams as ctc_beam_search_device returns them: (tokens [B, P, L] 0 padded, lengths [B, P], log_prob [B, P])"""
        _, top_paths, _ = _beam_args("tfasr_ctc_beam_nbest", self.V, self.beam_width, top_paths or self.beam_width, self.blank_index)
        dev, width, B = self.ws.device, self._width(), self.B
        tokens, lengths, log_prob = _paths(B, top_paths, width, dev)
        check(_L().tfasr_ctc_beam_nbest(*self._dims(), top_paths, width, _p(tokens), _p(lengths), _p(log_prob), _p(self.ws),
                                        self.ws.numel(), _stream()), "ctc_beam_nbest")
        return tokens, lengths, log_prob


class CtcLmBeamStream(_BeamStream):
    """The fused prefix beam search of ctc_beam_search_lm in pieces (tfasr_ctc_beam_lm_reset / _advance / _commit / _commit_horizon /
    _compact / _nbest): CtcBeamStream's interface with the n-gram tables `tables` = NGramLM.tables(alpha, beta), which every call of
    this object passes on (the carried LM states are node ids of these tables).  After any sequence of advances stream b holds the
    beam ctc_beam_search_lm holds after the same frames.  blank_index is the model's blank (the tables were built for it), never
    defaulted to V-1.  The streams in `final_rows` (commit, nbest) have ended and rank with the end-of-sentence term; the others rank
    by acoustic total + lm.  1 <= beam_width <= 32."""
    what = "tfasr_ctc_beam_lm_advance"

    def __init__(self, B, C, Tcap, V, beam_width, tables, blank_index=0, device="cuda"):
        self.C = int(C)
        self.beam_width, _, self.blank_index = _lm_beam_args(self.what, V, beam_width, 1, blank_index, tables)
        if not 1 <= self.C <= int(Tcap):
            raise ValueError(f"{self.what}: chunk capacity {self.C} outside [1, Tcap = {Tcap}]")
        self._init_common(B, Tcap, V, beam_width, device)
        self.tables = tables
        n = ctypes.c_size_t(0)
        check(_L().tfasr_ctc_beam_lm_stream_workspace_size(*self._dims(), ctypes.byref(n)), "ctc_beam_lm_stream_ws")
        self.ws = torch.empty(n.value, dtype=torch.uint8, device=device)
        self._lm = ctypes.addressof(_lm_device(tables, self.ws.device))
        self.reset()

    def _dims(self):
        return self.B, self.C, self.Tcap, self.V, self.beam_width

    def reset(self, rows=None):
        rows = None if rows is None else list(rows)
        mask = _row_mask(rows, self.B, self.ws.device)
        check(_L().tfasr_ctc_beam_lm_reset(_p(mask), *self._dims(), self._lm, _p(self.ws), self.ws.numel(), _stream()), "ctc_beam_lm_reset")
        self._reset_host(rows)

    def advance(self, logits, nvalid):
        """logits [B, Cn <= C, V] f32 / bf16 (device), nvalid [B] host values in [0, Cn]"""
        if logits.dim() != 3 or logits.shape[0] != self.B or logits.shape[2] != self.V or not 1 <= logits.shape[1] <= self.C:
            raise ValueError(f"ctc_beam_lm_advance: logits {tuple(logits.shape)}, expected [{self.B}, <= {self.C}, {self.V}]")
        Cn = int(logits.shape[1])
        nv, after = self._take(nvalid, Cn)
        logits = logits.contiguous()
        B, C, Tcap, V, W = self._dims()
        check(_L().tfasr_ctc_beam_lm_advance(_p(logits), _p(_i32(nv, self.ws.device)), B, C, Cn, Tcap, V, W, self.blank_index, _dt(logits),
                                             after, self._lm, _p(self.ws), self.ws.numel(), _stream()), "ctc_beam_lm_advance")
        self.frames = [f + v for f, v in zip(self.frames, nv)]

    def _commit(self, fin, tokens, n, width):
        check(_L().tfasr_ctc_beam_lm_commit(fin, _p(self.committed), tokens, n, *self._dims(), width, self._lm, _p(self.ws), self.ws.numel(),
                                            _stream()), "ctc_beam_lm_commit")

    def _commit_horizon(self, fin, tokens, n, width):
        check(_L().tfasr_ctc_beam_lm_commit_horizon(fin, _p(self.committed), tokens, n, _p(self.hstate), self.horizon, *self._dims(), width,
                                                    self._lm, _p(self.ws), self.ws.numel(), _stream()), "ctc_beam_lm_commit_horizon")

    def _compact(self, mask, hstate, horizon, out):
        check(_L().tfasr_ctc_beam_lm_compact(mask, _p(self.committed), hstate, horizon, out, *self._dims(), _p(self.ws), self.ws.numel(),
                                             _stream()), "ctc_beam_lm_compact")

    def nbest(self, top_paths=None, final_rows=None):
        """the current beams as ctc_beam_search_lm returns them: (tokens [B, P, L] 0 padded, lengths, score, log_prob, lm_score [B, P]);
        final_rows = the streams that have ended (None / empty: none)"""
        _, top_paths, _ = _beam_args("tfasr_ctc_beam_lm_nbest", self.V, self.beam_width, top_paths or self.beam_width, self.blank_index)
        dev, width, B = self.ws.device, self._width(), self.B
        final_rows = list(final_rows) if final_rows is not None else []
        fin = _row_mask(final_rows, B, dev) if final_rows else None
        tokens, lengths, score = _paths(B, top_paths, width, dev)
        log_prob, lm_score = torch.empty_like(score), torch.empty_like(score)
        check(_L().tfasr_ctc_beam_lm_nbest(_p(fin), *self._dims(), top_paths, width, _p(tokens), _p(lengths), _p(score), _p(log_prob),
                                           _p(lm_score), self._lm, _p(self.ws), self.ws.numel(), _stream()), "ctc_beam_lm_nbest")
        return tokens, lengths, score, log_prob, lm_score


def ctc_greedy_decode(logits, logit_len, blank=0):
    B, T, V = logits.shape
    am = torch.empty(B * T, dtype=torch.int32, device=logits.device)
    tokens = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    tlen = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(_L().tfasr_ctc_greedy_decode(_p(logits), _p(logit_len), _p(am), _p(tokens), _p(tlen), B, T, V, blank, _dt(logits), _stream()), "ctc_greedy")
    return tokens, tlen


def ctc_greedy_decode_detail(logits, logit_len, blank=0):
    """ctc_greedy_decode with spans and confidences: (tokens [B,T], tokens_len [B], starts [B,T], ends [B,T], tok_logp [B,T], tok_entropy
    [B,T], score [B]); token i of row b holds the frames [starts, ends), -1 past tokens_len (include/tfasr_hip.h)."""
    B, T, V = logits.shape
    dev = logits.device
    ws = torch.empty(3 * B * T, dtype=torch.int32, device=dev)
    tokens, starts, ends = (torch.empty(B, T, dtype=torch.int32, device=dev) for _ in range(3))
    tok_logp, tok_entropy = (torch.empty(B, T, dtype=torch.float32, device=dev) for _ in range(2))
    tlen = torch.empty(B, dtype=torch.int32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    check(_L().tfasr_ctc_greedy_decode_detail(_p(logits), _p(logit_len), _p(ws), _p(tokens), _p(tlen), _p(starts), _p(ends), _p(tok_logp),
                                              _p(tok_entropy), _p(score), B, T, V, blank, _dt(logits), _stream()), "ctc_greedy_detail")
    return tokens, tlen, starts, ends, tok_logp, tok_entropy, score


# --------------------------------------------------------------------------------- native Conformer-block executor
def block_ctx():
    return ctypes.create_string_buffer(int(_L().tfasr_block_ctx_bytes()))


def block_workspace_sizes(cfg):
    a, b, c = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    check(_L().tfasr_block_workspace_sizes(ctypes.byref(cfg), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "block_workspace_sizes")
    return a.value, b.value, c.value


def block_fwd(cfg, params, io, ctx, phase):
    check(_L().tfasr_block_fwd(ctypes.byref(cfg), ctypes.byref(params), ctypes.byref(io), ctx, phase, _stream()), "block_fwd")


def block_bwd(cfg, params, io, ctx, phase):
    check(_L().tfasr_block_bwd(ctypes.byref(cfg), ctypes.byref(params), ctypes.byref(io), ctx, phase, _stream()), "block_bwd")


def launch_count():
    """kernel launches the library has queued since it was loaded (tfasr_launch_count)"""
    return int(_L().tfasr_launch_count())


def block_side_stream():
    """the block executor's low-priority second stream (tfasr_block_side_stream) as a raw hipStream_t value"""
    ptr = ctypes.c_void_p(0)
    check(_L().tfasr_block_side_stream(ctypes.byref(ptr)), "block_side_stream")
    return int(ptr.value)


def block_wgrad_probe(enable):
    check(_L().tfasr_block_wgrad_probe(int(bool(enable))), "block_wgrad_probe")


def block_wgrad_probe_read():
    """(summed milliseconds, launches) of the grouped weight-gradient launches recorded since the probe was enabled / last read"""
    ms, n = ctypes.c_float(0.0), ctypes.c_int(0)
    check(_L().tfasr_block_wgrad_probe_read(ctypes.byref(ms), ctypes.byref(n)), "block_wgrad_probe_read")
    return float(ms.value), int(n.value)


def block_bwd_left(ctx):
    """bit mask of what the last block_bwd with this ctx left to the caller (tfasr_block_bwd_left)"""
    return int(_L().tfasr_block_bwd_left(ctx))


def block_wgrad_join(slot_mask=3):
    """The current stream waits for the grouped weight-gradient launches queued on the executor's second stream (tfasr_block_io.wgrad_slot)."""
    check(_L().tfasr_block_wgrad_join(int(slot_mask), _stream()), "block_wgrad_join")


def block_ln_fold_all(ctxs, d):
    """One launch for the LayerNorm gamma / beta gradients of every block whose backward ran with io.ln_part_ext (tfasr_block_ln_fold_all)."""
    arr = (ctypes.c_void_p * len(ctxs))(*[ctypes.addressof(c) for c in ctxs])
    check(_L().tfasr_block_ln_fold_all(arr, len(ctxs), int(d), _stream()), "block_ln_fold_all")


def block_dwconv_wgrad_all(cfg, params, ctxs, dcvs, device):
    """Depthwise-conv weight / bias gradients of every block whose backward ran with io.dcv_keep: one launch pair (tfasr_block_dwconv_wgrad_all)."""
    need = ctypes.c_size_t(0)
    check(_L().tfasr_dwconv_bwd_weight_workspace_size(cfg.B, cfg.T, cfg.d, cfg.ksize, ctypes.byref(need)), "dwconv_bwd_weight_workspace_size")
    for b0 in range(0, len(ctxs), 32):  # (at most 32 blocks per launch pair: deeper encoders take several)
        n = min(32, len(ctxs) - b0)
        ws = workspace(n * need.value, device, "dw_wgrad_all")
        pa = (ctypes.c_void_p * n)(*[ctypes.addressof(p) for p in params[b0:b0 + n]])
        ca = (ctypes.c_void_p * n)(*[ctypes.addressof(c) for c in ctxs[b0:b0 + n]])
        da = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dcvs[b0:b0 + n]])
        check(_L().tfasr_block_dwconv_wgrad_all(ctypes.byref(cfg), pa, ca, da, n, _p(ws), ws.numel(), _stream()), "block_dwconv_wgrad_all")


def layernorm_bwd_part_blocks(rows, C, dtype):
    return int(_L().tfasr_layernorm_bwd_part_blocks(int(rows), int(C), {torch.float32: 0, torch.bfloat16: 1}[dtype] if not isinstance(dtype, int) else dtype))


# --------------------------------------------------------------------------------- ContextNet pieces
def rows_subsample_fwd(x, stride):
    B, T, C = x.shape
    y = torch.empty(B, -(-T // stride), C, dtype=x.dtype, device=x.device)
    check(_L().tfasr_rows_subsample_fwd(_p(x), _p(y), B, T, C, stride, _dt(x), _stream()), "rows_subsample_fwd")
    return y


def rows_subsample_bwd(dy, T, stride):
    B, T2, C = dy.shape
    dx = torch.empty(B, T, C, dtype=dy.dtype, device=dy.device)
    check(_L().tfasr_rows_subsample_bwd(_p(dy), _p(dx), B, T, C, stride, _dt(dy), _stream()), "rows_subsample_bwd")
    return dx


def se_pool(x, lengths):
    B, T, C = x.shape
    pool = torch.empty(B, C, dtype=torch.float32, device=x.device)
    check(_L().tfasr_se_pool(_p(x), _p(lengths), _p(pool), B, T, C, _dt(x), _stream()), "se_pool")
    return pool


def se_scale_fwd(x, scale):
    B, T, C = x.shape
    y = torch.empty_like(x)
    check(_L().tfasr_se_scale_fwd(_p(x), _p(scale), _p(y), B, T, C, _dt(x), _stream()), "se_scale_fwd")
    return y


def se_scale_bwd_reduce(x, dy):
    B, T, C = x.shape
    ds = torch.empty(B, C, dtype=torch.float32, device=x.device)
    check(_L().tfasr_se_scale_bwd_reduce(_p(x), _p(dy), _p(ds), B, T, C, _dt(x), _stream()), "se_scale_bwd_reduce")
    return ds


def se_bwd_apply(dy, scale, dpool, lengths):
    B, T, C = dy.shape
    dx = torch.empty_like(dy)
    check(_L().tfasr_se_bwd_apply(_p(dy), _p(scale), _p(dpool), _p(lengths), _p(dx), B, T, C, _dt(dy), _stream()), "se_bwd_apply")
    return dx


def add_act_fwd(a, b, act=ACT_NONE):
    y = torch.empty_like(a)
    check(_L().tfasr_add_act_fwd(_p(a), _p(b), _p(y), a.numel(), act, _dt(a), _stream()), "add_act_fwd")
    return y


def add_act_bwd(a, b, dy, act=ACT_NONE):
    d = torch.empty_like(a)
    check(_L().tfasr_add_act_bwd(_p(a), _p(b), _p(dy), _p(d), a.numel(), act, _dt(a), _stream()), "add_act_bwd")
    return d


# ------------------------------------------------------------------------------------------- streaming (csrc/stream.hip)
STREAM_MAX_CHUNK, STREAM_MAX_KEYS, STREAM_MAX_HEAD = 32, 512, 128  # TFASR_STREAM_MAX_* of include/tfasr_hip.h


def stream_attn_fwd(qkv, ubias, vbias, pos, kcache, vcache, seen, nvalid, B, C, H, dh, hist, scale, out=None):
    """Chunk attention against the key / value rings: qkv [B*C, 3*H*dh], pos [hist + 2C - 1, H*dh], kcache / vcache [B, hist, H*dh],
    seen / nvalid [B] int32 on the device -> context [B*C, H*dh] (rows >= nvalid zero)."""
    if out is None:
        out = torch.empty(B * C, H * dh, dtype=qkv.dtype, device=qkv.device)
    st = _L().tfasr_stream_attn_fwd(_p(qkv), _p(ubias), _p(vbias), _p(pos), _p(kcache), _p(vcache), _p(seen), _p(nvalid), _p(out), B, C, H, dh,
                                    hist, scale, _dt(qkv), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"stream_attn_fwd: chunk {C} / keys {hist + C} / head {dh} beyond the kernel's limits "
                                    f"({STREAM_MAX_CHUNK}, {STREAM_MAX_KEYS}, {STREAM_MAX_HEAD})")
    check(st, "stream_attn_fwd")
    return out


def stream_kv_append(qkv, kcache, vcache, seen, nvalid, B, C, H, dh, hist):
    """The chunk's valid key / value rows into ring slots (seen + r) % hist; queue after stream_attn_fwd of the same layer."""
    check(_L().tfasr_stream_kv_append(_p(qkv), _p(kcache), _p(vcache), _p(seen), _p(nvalid), B, C, H, dh, hist, _dt(qkv), _stream()),
          "stream_kv_append")


def stream_attn_plain_fwd(qkv, kcache, vcache, seen, nvalid, B, C, H, dh, hist, scale, causal=False, out=None):
    """Plain chunk attention against the key / value rings AND the ring append, one launch: qkv [B*C, 3*H*dh] (a 2-D view whose rows are
    contiguous with stride 3*H*dh may start anywhere), kcache / vcache [B, hist, H*dh] (None with hist == 0), seen / nvalid [B] int32 on
    the device -> context [B*C, H*dh] (rows >= nvalid zero); the chunk's valid k / v rows are in the rings afterwards."""
    if out is None:
        out = torch.empty(B * C, H * dh, dtype=qkv.dtype, device=qkv.device)
    if qkv.dim() != 2 or qkv.shape != (B * C, 3 * H * dh) or qkv.stride() != (3 * H * dh, 1):
        raise _lib.TfasrError(f"stream_attn_plain_fwd: qkv {tuple(qkv.shape)} strides {qkv.stride()} is not [B*C, 3*H*dh] with contiguous rows")
    st = _L().tfasr_stream_attn_plain_fwd(_pv(qkv), _p(kcache), _p(vcache), _p(seen), _p(nvalid), _p(out), B, C, H, dh, hist, scale,
                                          1 if causal else 0, _dt(qkv), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"stream_attn_plain_fwd: chunk {C} / keys {hist + C} / head {dh} / batch {B} beyond the kernel's limits "
                                    f"({STREAM_MAX_CHUNK}, {STREAM_MAX_KEYS}, {STREAM_MAX_HEAD}, 65535)")
    check(st, "stream_attn_plain_fwd")
    return out


def stream_add_pe(x, pe, seen, nvalid, y=None):
    """y[b, r, :] = x[b, r, :] + pe[seen[b] + r, :] for r < nvalid[b], other rows copied: x [B, C, d] (f32 | bf16), pe [Tcap, d] f32; y may
    be x.  A valid row at or past Tcap becomes NaN (the table is never read past its end)."""
    B, C, d = x.shape
    assert pe.dtype == torch.float32 and pe.dim() == 2 and pe.shape[1] == d
    if y is None:
        y = torch.empty_like(x)
    check(_L().tfasr_stream_add_pe(_p(x), _p(pe), _p(seen), _p(nvalid), _p(y), B, C, d, pe.shape[0], _dt(x), _stream()), "stream_add_pe")
    return y


def stream_glu_dwconv_fwd(glu_x, state, w, bias, nvalid, B, C, out=None):
    """GLU + causal depthwise conv over state [B, K-1, d] ++ the chunk's valid rows; glu_x [B*C, 2d] -> [B*C, d]; state updated in place."""
    d = glu_x.shape[-1] // 2
    if out is None:
        out = torch.empty(B * C, d, dtype=glu_x.dtype, device=glu_x.device)
    check(_L().tfasr_stream_glu_dwconv_fwd(_p(glu_x), _p(state), _p(w), _p(bias), _p(nvalid), _p(out), B, C, d, w.shape[0], _dt(glu_x),
                                           _stream()), "stream_glu_dwconv_fwd")
    return out


def stream_rowconv_fwd(x, state, w, scale, shift, nvalid, B, C, out=None):
    """DeepSpeech2's RowConv1D over one step: causal depthwise conv without bias over state [B, K-1, d] ++ the valid rows of x [B*C, d], then
    * scale + shift (the folded BatchNorm) and the ReLU -> [B*C, d], rows >= nvalid zero; state updated in place.  The valid rows are the
    bits of dwconv_fwd -> channel_affine_fwd(relu=True) over the whole sequence."""
    d, Kt = x.shape[-1], w.shape[0]
    assert w.dtype == scale.dtype == shift.dtype == torch.float32 and w.shape[1] == d and scale.numel() == d and shift.numel() == d
    assert nvalid.dtype == torch.int32 and nvalid.numel() == B and x.numel() == B * C * d and x.is_contiguous()
    assert Kt == 1 or (state.shape == (B, Kt - 1, d) and state.dtype == x.dtype and state.is_contiguous())
    if out is None:
        out = torch.empty(B * C, d, dtype=x.dtype, device=x.device)
    st = _L().tfasr_stream_rowconv_fwd(_p(x), _p(state), _p(w), _p(scale), _p(shift), _p(nvalid), _p(out), B, C, d, Kt, _dt(x), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"stream_rowconv_fwd: {C} rows / {Kt} taps beyond {STREAM_MAX_CHUNK} rows a step, 32 taps")
    check(st, "stream_rowconv_fwd")
    return out


def logmel_stream(signal, nlen, prev, has_prev, T0, window, melw, band, frame_step, nfft, preemph, eps, out_dtype):
    """tfasr_logmel on the unconsumed samples of B streams: signal [B, N] f32, nlen [B] real samples per row, prev / has_prev [B] the sample
    in front of column 0 -> [B, T0, F]."""
    B, N = signal.shape
    F = melw.shape[1]
    out = torch.empty(B, T0, F, dtype=out_dtype, device=signal.device)
    assert signal.dtype == torch.float32 and prev.dtype == torch.float32
    check(_L().tfasr_logmel_stream(_p(signal), _p(nlen), _p(prev), _p(has_prev), B, N, preemph, _p(window), window.numel(), frame_step, nfft,
                                   _p(melw), _p(band), F, eps, _p(out), T0, _dt(out), _stream()), "logmel_stream")
    return out


def ctc_greedy_decode_carry(logits, logit_len, last_class, blank=0):
    """ctc_greedy_decode of one chunk per stream; last_class [B] int32 (in / out, -1 = none) carries the merge of repeats over the boundary."""
    B, T, V = logits.shape
    ws = torch.empty(B * T, dtype=torch.int32, device=logits.device)
    tokens = torch.empty(B, T, dtype=torch.int32, device=logits.device)
    tlen = torch.empty(B, dtype=torch.int32, device=logits.device)
    check(_L().tfasr_ctc_greedy_decode_carry(_p(logits), _p(logit_len), _p(last_class), _p(ws), _p(tokens), _p(tlen), B, T, V, blank,
                                             _dt(logits), _stream()), "ctc_greedy_decode_carry")
    return tokens, tlen


class CtcDetailState:
    """What tfasr_ctc_greedy_decode_carry_detail carries per stream (include/tfasr_hip.h): ints [B, 4] = previous class (-1: none), frames
    seen, a token is open, its first frame; floats [B, 3] = the open token's log-probability sum, its entropy sum, the path score."""

    def __init__(self, B, device="cuda"):
        self.B = int(B)
        self.ints = torch.empty(self.B, 4, dtype=torch.int32, device=device)
        self.floats = torch.empty(self.B, 3, dtype=torch.float32, device=device)
        self.reset()

    def reset(self, rows=None):
        r = slice(None) if rows is None else torch.as_tensor(list(rows), dtype=torch.long, device=self.ints.device)
        self.ints[r] = 0
        self.ints[r, 0] = -1
        self.floats[r] = 0

    @property
    def seen(self):
        return self.ints[:, 1]

    @property
    def open(self):
        return self.ints[:, 2] != 0

    @property
    def score(self):
        return self.floats[:, 2]


def ctc_greedy_decode_carry_detail(logits, logit_len, state, final=None, blank=0, packed=False):
    """One chunk [B, C, V] per stream with spans and confidences, one launch; `state` (CtcDetailState) is carried in place, final [B]
    int32 (default: none) closes the rows' open tokens.  -> (tokens, tokens_len [B], starts, ends, tok_logp, tok_entropy), all [B, C + 1]:
    column 0 = the token open on entry, columns 1 .. tokens_len = the tokens that start in this chunk, frames counted from the stream's
    reset, ends = -1 for a token still open (include/tfasr_hip.h).  packed=True: the same as ([3, B, C + 1] int32 = tokens, starts, ends;
    [2, B, C + 1] f32 = tok_logp, tok_entropy; tokens_len)."""
    B, C, V = logits.shape
    dev = logits.device
    if state.B != B or state.ints.device != dev:
        raise ValueError(f"ctc_greedy_decode_carry_detail: a state of {state.B} streams on {state.ints.device} for {B} rows on {dev}")
    if final is None:
        final = torch.zeros(B, dtype=torch.int32, device=dev)
    for t, what in ((logit_len, "logit_len"), (final, "final")):
        if t.dtype != torch.int32 or t.numel() != B or not t.is_contiguous():
            raise ValueError(f"ctc_greedy_decode_carry_detail: {what} is a contiguous int32 tensor of {B} rows")
    ibuf = torch.empty(3, B, C + 1, dtype=torch.int32, device=dev)  # tokens, starts, ends
    fbuf = torch.empty(2, B, C + 1, dtype=torch.float32, device=dev)  # tok_logp, tok_entropy
    tokens, starts, ends, tok_logp, tok_entropy = ibuf[0], ibuf[1], ibuf[2], fbuf[0], fbuf[1]
    tlen = torch.empty(B, dtype=torch.int32, device=dev)
    check(_L().tfasr_ctc_greedy_decode_carry_detail(_p(logits), _p(logit_len), _p(final), _p(state.ints), _p(state.floats), _p(tokens), _p(tlen),
                                                    _p(starts), _p(ends), _p(tok_logp), _p(tok_entropy), B, C, V, blank, _dt(logits), _stream()),
          "ctc_greedy_decode_carry_detail")
    if packed:  # (a session fetches two buffers instead of five)
        return ibuf, fbuf, tlen
    return tokens, tlen, starts, ends, tok_logp, tok_entropy


# ------------------------------------------------------------------------------------------- causal dense Conv1D (csrc/conv1d.hip)
def _conv1d_check(st, what):
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"{what}: outside 1 <= K <= 32, stride 1 | 2, (K - 1) * dilation <= 256, Cin % 16 == Cout % 16 == 0 "
                                    "(see include/tfasr_hip.h)")
    check(st, what)


def conv1d_workspace_size(B, T, Cin, Cout, K, stride=1, dilation=1, dtype=TFASR_F32):
    """Bytes of caller-owned workspace tfasr_conv1d_fwd needs for this shape (answers without a device)."""
    n = ctypes.c_size_t(0)
    _conv1d_check(_L().tfasr_conv1d_workspace_size(B, T, Cin, Cout, K, stride, dilation, dtype, ctypes.byref(n)), "conv1d_workspace_size")
    return n.value


def conv1d_pack_weight(w):
    """Keras Conv1D kernel [K, Cin, Cout] f32 (device) -> the packed bf16 copy the MFMA kernel's B operand reads (once per weight load)."""
    K, Cin, Cout = w.shape
    n = ctypes.c_size_t(0)
    _conv1d_check(_L().tfasr_conv1d_packed_weight_elems(K, Cin, Cout, ctypes.byref(n)), "conv1d_packed_weight_elems")
    out = torch.empty(n.value, dtype=torch.bfloat16, device=w.device)
    assert w.dtype == torch.float32
    _conv1d_check(_L().tfasr_conv1d_pack_weight(_p(w), _p(out), K, Cin, Cout, _stream()), "conv1d_pack_weight")
    return out


def conv1d_fwd(x, w, shape, bias=None, scale=None, shift=None, addend=None, relu=False, stride=1, dilation=1, lead=0, out=None):
    """Causal Conv1D: x [B, lead + T, Cin] (f32 | bf16) -> [B, ceil(T / stride), Cout]; shape = (K, Cin, Cout).  w: the Keras kernel
    (f32 activations) or conv1d_pack_weight's copy (bf16 activations).  Epilogue (acc + bias) * scale + shift [+ addend] [ReLU] in f32."""
    K, Cin, Cout = (int(v) for v in shape)
    B, rows = x.shape[0], x.shape[1]
    T = rows - int(lead)
    assert x.dim() == 3 and x.shape[2] == Cin and T >= 0
    Tout = -(-T // stride) if stride > 0 else 0
    if out is None:
        out = torch.empty(B, Tout, Cout, dtype=x.dtype, device=x.device)
    assert w.dtype == x.dtype and (addend is None or (addend.shape == out.shape and addend.dtype == x.dtype))
    assert out.shape == (B, Tout, Cout) and out.dtype == x.dtype
    want = ctypes.c_size_t(K * Cin * Cout)
    if x.dtype != torch.float32:
        _conv1d_check(_L().tfasr_conv1d_packed_weight_elems(K, Cin, Cout, ctypes.byref(want)), "conv1d_packed_weight_elems")
    if w.numel() != want.value:
        raise _lib.TfasrError(f"conv1d_fwd: the kernel holds {w.numel()} elements, {want.value} expected for {(K, Cin, Cout)} in {x.dtype}")
    for v in (bias, scale, shift):
        assert v is None or (v.dtype == torch.float32 and v.numel() == Cout)
    nbytes = conv1d_workspace_size(B, T, Cin, Cout, K, stride, dilation, _dt(x))
    ws = workspace(nbytes, x.device, "conv1d") if nbytes else None
    _conv1d_check(_L().tfasr_conv1d_fwd(_p(x), _p(w), _p(bias), _p(scale), _p(shift), _p(addend), _p(out), B, T, int(lead), Cin, Cout, K, stride,
                                        dilation, 1 if relu else 0, _dt(x), _p(ws), nbytes, _stream()), "conv1d_fwd")
    return out


def conv1d_tail_update(window, nvalid, tail):
    """tail [B, n, C] <- rows nvalid[b] .. nvalid[b] + n - 1 of window [B, rows, C] (old tail ++ new rows); nvalid [B] int32 device."""
    B, rows, C = window.shape
    assert tail.shape[0] == B and tail.shape[2] == C and tail.dtype == window.dtype and nvalid.dtype == torch.int32
    check(_L().tfasr_conv1d_tail_update(_p(window), _p(nvalid), _p(tail), B, rows, tail.shape[1], C, _dt(window), _stream()), "conv1d_tail_update")
    return tail


# ------------------------------------------------------------------------------------------- general Conv2D (csrc/conv2d_gen.hip)
def _conv2d_check(st, what):
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"{what}: outside 1 <= kh <= 16, 1 <= kw <= 48, time stride 1..3, frequency stride 1 | 2, Cin = 1 or a "
                                    "multiple of 16 up to 128, Cout a multiple of 16 up to 128 (see include/tfasr_hip.h)")
    check(st, what)


def conv_pad_out(L, k, s, padding):
    """(left padding, output length) of one axis: "same" as keras (out = ceil(L / s), total = max((out - 1) s + k - L, 0), left = total // 2),
    "causal" as the reference's Conv2D (layers/convolution.py:132-144: k - 1 zeros in front, then "valid": out = ceil(L / s))."""
    L, k, s = int(L), int(k), int(s)
    out = -(-L // s)
    if padding == "same":
        return max((out - 1) * s + k - L, 0) // 2, out
    if padding == "causal":
        return k - 1, out
    raise ValueError(f"padding {padding!r}: 'same' or 'causal'")


def conv2d_pack_weight(w):
    """Keras Conv2D kernel [kh, kw, Cin, Cout] f32 (device) -> the packed bf16 copy the MFMA kernel reads (once per weight load)."""
    kh, kw, Cin, Cout = w.shape
    n = ctypes.c_size_t(0)
    _conv2d_check(_L().tfasr_conv2d_packed_weight_elems(kh, kw, Cin, Cout, ctypes.byref(n)), "conv2d_packed_weight_elems")
    out = torch.empty(n.value, dtype=torch.bfloat16, device=w.device)
    assert w.dtype == torch.float32
    _conv2d_check(_L().tfasr_conv2d_pack_weight(_p(w), _p(out), kh, kw, Cin, Cout, _stream()), "conv2d_pack_weight")
    return out


def conv2d_fwd(x, w, shape, bias=None, scale=None, shift=None, relu=False, strides=(1, 1), padding="same", out=None, lead=0):
    """Conv2D, channels-last: x [B, T, F, Cin] (f32 | bf16) -> [B, ceil(T / st), ceil(F / sf), Cout]; shape = (kh, kw, Cin, Cout); padding
    "same" or "causal" on both axes (conv_pad_out).  w: the Keras kernel (f32 activations) or conv2d_pack_weight's copy (bf16
    activations).  Epilogue (acc + bias) * scale + shift [ReLU] in f32.
    lead = kh - 1 (causal padding only): x is [tail | new rows], the first `lead` rows being real left context carried from the step in
    front (zeros at a stream's start) in place of the causal zero padding: the time axis is convolved "valid" and the output has
    ceil((T - lead) / st) rows, those of the new rows; the frequency axis keeps its causal padding."""
    kh, kw, Cin, Cout = (int(v) for v in shape)
    st, sf = (int(v) for v in strides)
    assert x.dim() == 4 and x.shape[3] == Cin
    B, T, F = x.shape[:3]
    (pad_t, To), (pad_f, Fo) = conv_pad_out(T, kh, st, padding), conv_pad_out(F, kw, sf, padding)
    lead = int(lead)
    if lead:
        if padding != "causal" or lead != kh - 1 or T < lead:
            raise ValueError(f"conv2d_fwd: lead = {lead} needs causal padding, lead == kh - 1 = {kh - 1} and at least that many rows")
        pad_t, To = 0, -(-(T - lead) // st)
    if out is None:
        out = torch.empty(B, To, Fo, Cout, dtype=x.dtype, device=x.device)
    assert w.dtype == x.dtype and out.shape == (B, To, Fo, Cout) and out.dtype == x.dtype
    want = ctypes.c_size_t(kh * kw * Cin * Cout)
    if x.dtype != torch.float32:
        _conv2d_check(_L().tfasr_conv2d_packed_weight_elems(kh, kw, Cin, Cout, ctypes.byref(want)), "conv2d_packed_weight_elems")
    if w.numel() != want.value:
        raise _lib.TfasrError(f"conv2d_fwd: the kernel holds {w.numel()} elements, {want.value} expected for {(kh, kw, Cin, Cout)} in {x.dtype}")
    for v in (bias, scale, shift):
        assert v is None or (v.dtype == torch.float32 and v.numel() == Cout)
    if B == 0 or To == 0 or Fo == 0:
        return out
    n = ctypes.c_size_t(0)
    _conv2d_check(_L().tfasr_conv2d_workspace_size(B, T, F, To, Fo, Cin, Cout, kh, kw, st, sf, pad_t, pad_f, _dt(x), ctypes.byref(n)),
                  "conv2d_workspace_size")
    ws = workspace(n.value, x.device, "conv2d") if n.value else None
    _conv2d_check(_L().tfasr_conv2d_fwd(_p(x), _p(w), _p(bias), _p(scale), _p(shift), _p(out), B, T, F, To, Fo, Cin, Cout, kh, kw, st, sf, pad_t,
                                        pad_f, 1 if relu else 0, _dt(x), _p(ws), n.value, _stream()), "conv2d_fwd")
    return out


def channel_affine_fwd(x, scale=None, shift=None, relu=False, y=None):
    """y = x * scale[c] + shift[c] over the last axis, ReLU when asked (an inference BatchNorm + activation; f32 vectors)."""
    rows, C = x.numel() // x.shape[-1], x.shape[-1]
    if y is None:
        y = torch.empty_like(x)
    check(_L().tfasr_channel_affine_fwd(_p(x), _p(scale), _p(shift), _p(y), rows, C, 1 if relu else 0, _dt(x), _stream()), "channel_affine_fwd")
    return y


# ------------------------------------------------------------------------------------------- inference LSTM (csrc/lstm_infer.hip)
def lstm_infer_workspace_size(B, T, P, ndir=1, dtype=TFASR_F32):
    n = ctypes.c_size_t(0)
    check(_L().tfasr_lstm_infer_workspace_size(B, T, P, ndir, dtype, ctypes.byref(n)), "lstm_infer_workspace_size")
    return n.value


def lstm_infer_fwd(xg, rk, lengths=None, ndir=1, y=None, want_state=False, ws=None, state=None, state_out=None):
    """The inference recurrence of one (ndir 1) or two (ndir 2: keras Bidirectional, concat) LSTMs over xg [B, T, ndir * 4P] (input
    projections of the directions side by side), rk [ndir, P, 4P], lengths [B] int32 (device) or None -> y [B, T, ndir * P]; with
    want_state also (h_last, c_last) [ndir, B, P] f32.  One persistent launch where the shape allows it, else the per-step kernels
    (tfasr_lstm_infer_fwd decides).  ws: a uint8 workspace to use (its first ndir * 16 int32 words are the directions' {count, abort}
    records, read by tests); default: the shared grow-only one.
    state = (h0, c0) [B, P] f32: the recurrence continues from it (one direction only; tfasr_lstm_infer_fwd_state) - the h_last / c_last
    of the call over the frames in front of these.  state_out = (h_last, c_last) [B, P] f32 buffers to fill, which must not be the
    state's own (the library refuses aliases: callers ping-pong two pairs); they are returned as with want_state, shaped as given."""
    B, T, G = xg.shape
    P = G // (4 * ndir)
    assert G == ndir * 4 * P and rk.numel() == ndir * P * 4 * P and rk.dtype == xg.dtype and xg.is_contiguous()
    assert lengths is None or (lengths.dtype == torch.int32 and lengths.numel() == B)
    if y is None:
        y = torch.empty(B, T, ndir * P, dtype=xg.dtype, device=xg.device)
    assert y.shape == (B, T, ndir * P) and y.dtype == xg.dtype
    h_last = c_last = h0 = c0 = None
    if state_out is not None:
        h_last, c_last = state_out
        want_state = True
        for t in (h_last, c_last):
            assert t.dtype == torch.float32 and t.numel() == ndir * B * P and t.is_contiguous() and t.device == xg.device
    elif want_state:
        h_last = torch.empty(ndir, B, P, dtype=torch.float32, device=xg.device)
        c_last = torch.empty(ndir, B, P, dtype=torch.float32, device=xg.device)
    if state is not None:
        h0, c0 = state
        for t in (h0, c0):
            assert t.dtype == torch.float32 and t.shape == (B, P) and t.is_contiguous() and t.device == xg.device
    if B == 0 or T == 0:
        if state is not None and want_state:
            h_last.view(B, P).copy_(h0)
            c_last.view(B, P).copy_(c0)
        return (y, h_last, c_last) if want_state else y
    nbytes = lstm_infer_workspace_size(B, T, P, ndir, _dt(xg))
    if ws is None:
        ws = workspace(nbytes, xg.device, "lstm_infer")
    assert ws.numel() >= nbytes
    if state is None:
        check(_L().tfasr_lstm_infer_fwd(_p(xg), G, _p(rk), _p(lengths), _p(y), ndir * P, _p(h_last), _p(c_last), B, T, P, ndir, _dt(xg), _p(ws),
                                        ws.numel(), _stream()), "lstm_infer_fwd")
    else:
        check(_L().tfasr_lstm_infer_fwd_state(_p(xg), G, _p(rk), _p(lengths), _p(y), ndir * P, _p(h0), _p(c0), _p(h_last), _p(c_last), B, T, P,
                                              ndir, _dt(xg), _p(ws), ws.numel(), _stream()), "lstm_infer_fwd_state")
    return (y, h_last, c_last) if want_state else y


# ------------------------------------------------------------------------------------------- plain attention (csrc/attn_plain.hip)
def attn_plain_fwd(qkv, lengths, B, H, T, dh, scale, use_mask=True, causal=False, chunk_size=None, history_size=None, want_lse=False, out=None):
    """Fused scaled dot-product attention of the Transformer encoder: qkv [B*T, 3*H*dh] (q|k|v column blocks) -> out [B*T, H*dh]
    (and lse [B, H, T] f32 when asked).  Padded query rows (use_mask, i >= lengths[b]) attend uniformly over all T keys; keys are never
    masked by length; causal = the lower triangle; chunk_size / history_size = the streaming window of relattn_fused_fwd.
    bf16: dh 64 | 128; f32: dh % 16 == 0, dh <= 128; anything else raises TfasrUnsupported and launches nothing."""
    assert qkv.dim() == 2 and qkv.shape == (B * T, 3 * H * dh)
    if out is None:
        out = torch.empty(B * T, H * dh, dtype=qkv.dtype, device=qkv.device)
    assert out.shape == (B * T, H * dh) and out.dtype == qkv.dtype
    lse = torch.empty(B, H, T, dtype=torch.float32, device=qkv.device) if want_lse else None
    ck, hs = _window(chunk_size, history_size)
    st = _L().tfasr_attn_plain_fwd(_p(qkv), _p(lengths), _p(out), _p(lse), B, H, T, dh, float(scale), 1 if use_mask else 0, 1 if causal else 0,
                                   ck, hs, _dt(qkv), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"attn_plain_fwd: head size {dh} in {qkv.dtype}: bf16 takes 64 | 128, f32 a multiple of 16 up to 128")
    check(st, "attn_plain_fwd")
    return (out, lse) if want_lse else out


def add_pe(x, pe, lengths=None, y=None):
    """y[b, t, :] = x[b, t, :] + (t < lengths[b] ? pe[t, :] : 0): x [B, T, d] (f32 | bf16), pe [T, d] f32; y may be x."""
    B, T, d = x.shape
    assert pe.dtype == torch.float32 and pe.shape == (T, d)
    if y is None:
        y = torch.empty_like(x)
    check(_L().tfasr_add_pe(_p(x), _p(pe), _p(lengths), _p(y), B, T, d, _dt(x), _stream()), "add_pe")
    return y


# ------------------------------------------------------------------------------------------- RnnTransducerBlock tail (csrc/rnnt_block.hip)
def rnnt_block_tail_supported(P, N):
    """the range of tfasr_rnnt_block_tail_fwd (include/tfasr_hip.h); outside it callers run layernorm_fwd + gemm"""
    return P % 32 == 0 and 0 < P <= 2048 and N % 16 == 0 and 0 < N <= 1024


def rnnt_block_tail_fwd(y, gamma, beta, W, bias, N, lengths=None, off=None, factor=1, Tpad=None, out=None, out_lengths=None, eps=1e-3):
    """out[b, off_b + t, :] = LayerNorm(y[b, t, :]) W + bias in one launch: y [B, T, P] (f32 | bf16; a view whose rows are strided is
    fine), gamma / beta [P] f32, W the Keras kernel [P, N] f32 (f32 activations) or conv1d_pack_weight's copy of it as one tap (bf16),
    bias [N] f32 or None -> out [B, Tpad, N], Tpad (default: T rounded up) a multiple of `factor`.  Rows t >= lengths[b] are computed
    from zeros, rows [off_b + T, Tpad) are written as zeros, rows in front of off_b are left alone (pass `out` holding them);
    out_lengths [B] int32 receives ceil((off_b + min(lengths[b], T)) / factor).  Returns (out, out_lengths); raises TfasrUnsupported
    outside the kernel's range (rnnt_block_tail_supported) and launches nothing."""
    B, T, P = y.shape
    factor = max(int(factor), 1)
    if Tpad is None:
        Tpad = -(-T // factor) * factor
    assert y.stride(2) == 1 and (B <= 1 or y.stride(0) == T * y.stride(1)), "y: [B, T, P] with one row stride"
    assert gamma.dtype == torch.float32 and beta.dtype == torch.float32 and gamma.numel() == P and beta.numel() == P
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == N)
    assert W.dtype == y.dtype
    if rnnt_block_tail_supported(P, N):
        want = ctypes.c_size_t(P * N)
        if y.dtype != torch.float32:
            _conv1d_check(_L().tfasr_conv1d_packed_weight_elems(1, P, N, ctypes.byref(want)), "conv1d_packed_weight_elems")
        if W.numel() != want.value:
            raise _lib.TfasrError(f"rnnt_block_tail_fwd: the kernel holds {W.numel()} elements, {want.value} expected for {(P, N)} in {y.dtype}")
    for v in (lengths, off):
        assert v is None or (v.dtype == torch.int32 and v.numel() == B)
    if out is None:
        out = torch.empty(B, Tpad, N, dtype=y.dtype, device=y.device)
    assert out.shape == (B, Tpad, N) and out.dtype == y.dtype
    if out_lengths is None:
        out_lengths = torch.empty(B, dtype=torch.int32, device=y.device)
    assert out_lengths.dtype == torch.int32 and out_lengths.numel() == B
    st = _L().tfasr_rnnt_block_tail_fwd(_pv(y), y.stride(1), _p(lengths), _p(off), _p(gamma), _p(beta), _p(W), _p(bias), _p(out), _p(out_lengths),
                                        B, T, Tpad, P, N, factor, float(eps), _dt(y), _stream())
    if st == _lib.STATUS_UNSUPPORTED:
        raise _lib.TfasrUnsupported(f"rnnt_block_tail_fwd: P={P} N={N}: P % 32 == 0 up to 2048 and N % 16 == 0 up to 1024")
    check(st, "rnnt_block_tail_fwd")
    return out, out_lengths

